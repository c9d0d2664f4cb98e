// Whole-run snapshots (dctn_amd/checkpoint.py): ONE launch copies up to 16 device regions - the flat parameter buffer,
// the moments, the master copy, the 16- and 32-byte state blocks - into one contiguous arena (gather) or back in place
// (scatter), and leaves one digest per region.  include/dctn_amd.h holds the normative layout and digest.
//   layout : region r starts at 16 * (sum of ceil(bytes[q] / 16) over q < r); the padding is zero
//   digest : the region's bytes, zero-padded to 16, as little-endian uint32 words w_0 .. w_(m-1):
//            s1 = sum w_i, s2 = sum (i + 1) w_i, both mod 2^64 - integer sums, so every order gives the same bits
// The table of pointers and lengths travels by value in the kernel argument (core_dropout.hip's DropSegs): the launch
// reads no host memory and can be captured.
//
// Work is dealt in TILES of 4096 bytes = 256 lanes x one 16-byte chunk, and a tile never spans two regions (a region
// of n bytes has ceil(n / 4096) of them).  A workgroup takes STATE_UNROLL tiles per pass, a grid apart: it issues the
// loads of all of them, then the stores of all of them in one burst - loads and stores retire through one in-order
// counter on gfx950, so a store placed between two loads would make the second load's wait a wait for the store - and
// forms the digest behind the stores.  A lane keeps its partial (s1, s2) while its tiles stay in one region; when the
// region changes, and at the end, a wave adds its 64 partials by shuffles and its first lane adds the pair to the
// region's cells with two 64-bit vector atomics (the entry point zeroes the cells in front of the launch).  No
// workgroup waits for another.
#include "common.h"

namespace {

constexpr int STATE_MAX_REGIONS = 16;
constexpr int STATE_THREADS = 256;
constexpr int STATE_UNROLL = 4;
constexpr unsigned long long STATE_TILE_CHUNKS = STATE_THREADS;   // 16-byte chunks of a tile: one per lane

struct StateTable {   // passed by value in the kernel argument
  unsigned char* region[STATE_MAX_REGIONS];          // gather: read; scatter: written
  unsigned long long bytes[STATE_MAX_REGIONS];
  unsigned long long tile_end[STATE_MAX_REGIONS];    // running total of tiles
  unsigned long long chunk_off[STATE_MAX_REGIONS];   // where the region starts in the arena, in 16-byte chunks
  int count;
};

__device__ __forceinline__ unsigned state_dword(const unsigned* q) {
  return __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
}

// Chunk at `p` of a region based at `base` with `rem` >= 1 bytes left from `p` on: 16-byte access when the region is
// aligned for it, dwords otherwise; the last chunk's whole dwords, then its last rem % 4 bytes as a short and / or a
// byte.  Nothing past the region's last byte is touched; what lies past it comes back as zero.
__device__ __forceinline__ uint4 state_load_region(const unsigned char* p, bool vec, unsigned long long rem) {
  if (rem >= 16) {
    if (vec) return *reinterpret_cast<const uint4*>(p);
    // relaxed wave-scope atomics are plain dword accesses that the compiler leaves apart: it would join four ordinary
    // ones into one 16-byte access at a 4-byte aligned address
    const unsigned* q = reinterpret_cast<const unsigned*>(p);
    return make_uint4(state_dword(q), state_dword(q + 1), state_dword(q + 2), state_dword(q + 3));
  }
  const unsigned full = (unsigned)rem >> 2, tail = (unsigned)rem & 3u;
  unsigned last = 0u;
  if (tail) {
    const unsigned char* b = p + 4 * full;
    if (tail == 1) last = b[0];
    else last = *reinterpret_cast<const unsigned short*>(b);
    if (tail == 3) last |= (unsigned)b[2] << 16;
  }
  unsigned v[4];
#pragma unroll
  for (unsigned j = 0; j < 4; ++j) {
    v[j] = 0u;
    if (j < full) v[j] = reinterpret_cast<const unsigned*>(p)[j];
    else if (j == full) v[j] = last;
  }
  return make_uint4(v[0], v[1], v[2], v[3]);
}

__device__ __forceinline__ void state_store_region(unsigned char* p, bool vec, unsigned long long rem, const uint4& w) {
  if (rem >= 16) {
    if (vec) {
      *reinterpret_cast<uint4*>(p) = w;
    } else {
      unsigned* q = reinterpret_cast<unsigned*>(p);   // kept as four dwords, as the loads are
      const unsigned v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
      for (int j = 0; j < 4; ++j) __hip_atomic_store(q + j, v[j], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WAVEFRONT);
    }
    return;
  }
  const unsigned full = (unsigned)rem >> 2, tail = (unsigned)rem & 3u;
  const unsigned v[4] = {w.x, w.y, w.z, w.w};
  unsigned last = 0u;
#pragma unroll
  for (unsigned j = 0; j < 4; ++j) {
    if (j < full) reinterpret_cast<unsigned*>(p)[j] = v[j];
    else if (j == full) last = v[j];
  }
  if (tail) {
    unsigned char* b = p + 4 * full;
    if (tail == 1) b[0] = (unsigned char)last;
    else *reinterpret_cast<unsigned short*>(b) = (unsigned short)last;
    if (tail == 3) b[2] = (unsigned char)(last >> 16);
  }
}

// the bytes of the arena's last chunk of a region that lie past the region (its padding) do not enter the digest
__device__ __forceinline__ uint4 state_mask(const uint4& w, unsigned long long rem) {
  if (rem >= 16) return w;
  unsigned v[4] = {w.x, w.y, w.z, w.w};
#pragma unroll
  for (unsigned j = 0; j < 4; ++j) {
    const unsigned have = (unsigned)rem > 4 * j ? (unsigned)rem - 4 * j : 0u;   // bytes of word j inside the region
    if (have == 0) v[j] = 0u;
    else if (have < 4) v[j] &= (1u << (8 * have)) - 1u;
  }
  return make_uint4(v[0], v[1], v[2], v[3]);
}

__device__ __forceinline__ void state_flush(unsigned long long* digests, int region, unsigned long long s1,
                                            unsigned long long s2) {
  if (region < 0) return;   // uniform over the workgroup
  s1 = wave_reduce_sum(s1);
  s2 = wave_reduce_sum(s2);
  if ((threadIdx.x & 63) == 0 && (s1 | s2)) {
    __hip_atomic_fetch_add(&digests[2 * region], s1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    __hip_atomic_fetch_add(&digests[2 * region + 1], s2, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

template <bool SCATTER>
__global__ __launch_bounds__(STATE_THREADS) void state_copy_k(StateTable tab, unsigned char* __restrict__ arena,
                                                              unsigned long long* __restrict__ digests) {
  const unsigned long long total = tab.tile_end[tab.count - 1];
  unsigned long long s1 = 0, s2 = 0;
  int cur = -1, s = 0;
  for (unsigned long long t0 = blockIdx.x; t0 < total; t0 += (unsigned long long)gridDim.x * STATE_UNROLL) {
    uint4 w[STATE_UNROLL];
    int reg[STATE_UNROLL];                 // region of the tile (uniform over the workgroup); -1: no tile
    unsigned long long chunk[STATE_UNROLL];   // this lane's chunk of the region
    unsigned long long rem[STATE_UNROLL];     // bytes of the region from that chunk on; 0: the lane has none
#pragma unroll
    for (int u = 0; u < STATE_UNROLL; ++u) {
      const unsigned long long t = t0 + (unsigned long long)u * gridDim.x;
      reg[u] = -1, rem[u] = 0, chunk[u] = 0, w[u] = make_uint4(0u, 0u, 0u, 0u);
      if (t >= total) continue;
      while (s < tab.count - 1 && t >= tab.tile_end[s]) ++s;   // tiles come in rising order
      reg[u] = s;
      chunk[u] = (t - (s ? tab.tile_end[s - 1] : 0ull)) * STATE_TILE_CHUNKS + threadIdx.x;
      const unsigned long long n = tab.bytes[s];
      if (chunk[u] * 16ull >= n) continue;
      rem[u] = n - chunk[u] * 16ull;
      if (SCATTER) {
        w[u] = *reinterpret_cast<const uint4*>(arena + (tab.chunk_off[s] + chunk[u]) * 16ull);
      } else {
        const unsigned char* base = tab.region[s];
        w[u] = state_load_region(base + chunk[u] * 16ull, ((uintptr_t)base & 15u) == 0, rem[u]);
      }
    }
#pragma unroll
    for (int u = 0; u < STATE_UNROLL; ++u) {
      if (rem[u] == 0) continue;
      if (SCATTER) {
        unsigned char* base = tab.region[reg[u]];
        state_store_region(base + chunk[u] * 16ull, ((uintptr_t)base & 15u) == 0, rem[u], w[u]);
      } else {   // the whole chunk: a region's last one carries the zero padding
        *reinterpret_cast<uint4*>(arena + (tab.chunk_off[reg[u]] + chunk[u]) * 16ull) = w[u];
      }
    }
#pragma unroll
    for (int u = 0; u < STATE_UNROLL; ++u) {
      if (reg[u] < 0) continue;
      if (reg[u] != cur) {
        state_flush(digests, cur, s1, s2);
        cur = reg[u], s1 = 0, s2 = 0;
      }
      if (rem[u] == 0) continue;
      const uint4 d = SCATTER ? state_mask(w[u], rem[u]) : w[u];
      const unsigned long long sum = (unsigned long long)d.x + d.y + d.z + d.w;
      s1 += sum;
      // words 4 c .. 4 c + 3 weigh 4 c + 1 .. 4 c + 4
      s2 += chunk[u] * 4ull * sum + ((unsigned long long)d.x + 2ull * d.y + 3ull * d.z + 4ull * d.w);
    }
  }
  state_flush(digests, cur, s1, s2);
}

// the table of a call, or the error code of include/dctn_amd.h; `padded` receives the arena's size
int state_table(StateTable& tab, void* const* regions, const int64_t* bytes, int n_regions, unsigned long long& padded) {
  if (!regions || !bytes) return DCTN_ERR_NULL;
  if (n_regions < 1) return DCTN_ERR_BAD_SHAPE;
  if (n_regions > STATE_MAX_REGIONS) return DCTN_ERR_UNSUPPORTED;
  for (int r = 0; r < n_regions; ++r)
    if (!regions[r]) return DCTN_ERR_NULL;
  unsigned long long chunks = 0, tiles = 0;
  for (int r = 0; r < n_regions; ++r) {
    if (bytes[r] < 1 || bytes[r] > (int64_t)1 << 46) return DCTN_ERR_BAD_SHAPE;
    const unsigned long long c = ((unsigned long long)bytes[r] + 15ull) / 16ull;
    tab.region[r] = static_cast<unsigned char*>(regions[r]);
    tab.bytes[r] = (unsigned long long)bytes[r];
    tab.chunk_off[r] = chunks;
    chunks += c;
    tiles += (c + STATE_TILE_CHUNKS - 1) / STATE_TILE_CHUNKS;
    tab.tile_end[r] = tiles;
  }
  tab.count = n_regions;
  padded = chunks * 16ull;
  return DCTN_OK;
}

template <bool SCATTER>
int state_launch(void* const* regions, const int64_t* bytes, int n_regions, void* arena, const size_t* arena_bytes,
                 void* digests, void* stream) {
  if (!arena || !digests) return DCTN_ERR_NULL;
  StateTable tab = {};
  unsigned long long padded = 0;
  const int rc = state_table(tab, regions, bytes, n_regions, padded);
  if (rc != DCTN_OK) return rc;
  if (arena_bytes && (unsigned long long)*arena_bytes != padded) return DCTN_ERR_BAD_SHAPE;
  for (int r = 0; r < n_regions; ++r)
    if ((uintptr_t)regions[r] % 4) return DCTN_ERR_UNSUPPORTED;
  if ((uintptr_t)arena % 16 || (uintptr_t)digests % 8) return DCTN_ERR_UNSUPPORTED;
  hipStream_t st = (hipStream_t)stream;
  const int zeroed = dctn_zero_async(digests, (size_t)n_regions * 16, st);   // the cells the launch adds into
  if (zeroed != DCTN_OK) return zeroed;
  const unsigned long long tiles = tab.tile_end[n_regions - 1];
  unsigned long long wgs = (tiles + STATE_UNROLL - 1) / STATE_UNROLL;
  const unsigned long long cap = 2ull * (unsigned long long)(dctn_dev().cus < 1 ? 1 : dctn_dev().cus);
  if (wgs > cap) wgs = cap;
  hipLaunchKernelGGL((state_copy_k<SCATTER>), dim3((unsigned)wgs), dim3(STATE_THREADS), 0, st, tab,
                     static_cast<unsigned char*>(arena), static_cast<unsigned long long*>(digests));
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

}  // namespace

extern "C" {

int dctn_state_max_regions(void) { return STATE_MAX_REGIONS; }

size_t dctn_state_arena_bytes(const int64_t* bytes, int n_regions) {
  if (!bytes || n_regions < 1 || n_regions > STATE_MAX_REGIONS) return 0;
  unsigned long long total = 0;
  for (int r = 0; r < n_regions; ++r) {
    if (bytes[r] < 1 || bytes[r] > (int64_t)1 << 46) return 0;
    total += ((unsigned long long)bytes[r] + 15ull) / 16ull * 16ull;
  }
  return (size_t)total;
}

int dctn_state_gather(const void* const* srcs, const int64_t* bytes, int n_regions, void* arena, size_t arena_bytes,
                      void* digests, void* stream) {
  return state_launch<false>(const_cast<void* const*>(srcs), bytes, n_regions, arena, &arena_bytes, digests, stream);
}

int dctn_state_scatter(const void* arena, void* const* dsts, const int64_t* bytes, int n_regions, void* digests,
                       void* stream) {
  return state_launch<true>(dsts, bytes, n_regions, const_cast<void*>(arena), nullptr, digests, stream);
}

}  // extern "C"
