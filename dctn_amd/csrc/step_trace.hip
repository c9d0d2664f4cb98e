// The step trace: ONE launch at the end of a training iteration that writes one 64-byte record - the loss, the rows of
// the batch and how many of them the model got right, and the gradient guard's, the optimizer's and the batch source's
// device blocks as they stand - into a ring on the device and advances a device counter.  A captured graph that holds the
// launch fills consecutive slots on its replays, so K iterations of one graph launch leave K records and the host reads
// them when it likes (include/dctn_amd.h holds the normative layout; dctn_amd/training.py `StepTrace` is the host side).
// ONE workgroup of 16 waves, as ce_score_k: B * C is ~1e4 values, the launch is latency (so every lane has eight loads in
// flight and the state blocks are fetched under the row loop), and with one workgroup nothing
// has to be handed between workgroups - no ticket is drawn (the head's ticket word stays 0), nobody waits.  The counts
// are integers: the record is the same bits from run to run.
#include "common.h"
#include "grad_guard.h"

#include <cmath>

namespace {

constexpr long long TRACE_IGNORE = -100;   // torch.nn.functional.cross_entropy's default ignore_index (ce_score_k's rule)

struct TraceHead {   // include/dctn_amd.h documents this layout: it is part of the ABI
  unsigned records_done, ticket, reserved0, reserved1;
};
static_assert(sizeof(TraceHead) == 16, "the trace head is 16 bytes (include/dctn_amd.h)");

struct TraceAdamState {   // lr_schedule.h's StepStateBlock
  int steps_done;
  float lr;
  unsigned ticket, reserved;
};

struct TraceBatchState {   // draw_order.h's BatchState
  unsigned seed_lo, seed_hi, batches_done, ticket;
};

constexpr int TRACE_RECORD_BYTES = 64;
constexpr unsigned TRACE_HAS_REG = 1u, TRACE_HAS_GUARD = 2u, TRACE_HAS_ADAM = 4u, TRACE_HAS_SOURCE = 8u;

__device__ __forceinline__ float tr_ld(const float* p) { return *p; }
__device__ __forceinline__ float tr_ld(const bf16_t* p) { return (float)*p; }

constexpr int TRACE_UNROLL = 8;   // a lane's loads in flight: the launch is a chain of round trips, not bandwidth

// The better of two (maximum, lowest index that holds it) pairs.  m is never NaN (see below), so == and > are total here.
__device__ __forceinline__ void tr_better(float& m, int& first, float m2, int first2) {
  if (m2 > m || (m2 == m && first2 < first)) m = m2, first = first2;
}

// dctn_ce_score_accumulate's row rules without its exponentials: the maximum by fmaxf - a NaN logit is never the maximum,
// and a row of nothing but NaN has none - and the LOWEST index that holds it (torch.argmax's answer on ties).  One pass:
// `x > m` keeps the first of equal values and drops a NaN; `first` unset and x == m is the row whose maximum is -inf.
// A row belongs to P = min(64, next power of two >= C / 8) neighbouring lanes; lane j of them holds classes j, j + P, ...
// and fetches EIGHT of them per round before it looks at any (the filler of a slot past C is a NaN, which the rules
// ignore); the pairs of a row's lanes are closed by xor butterflies.  cfg2's batch (1024 x 10) is P = 2, one round per
// lane and two passes of the workgroup: a per-row layout of 16 lanes and one class per lane was 16 passes of three
// dependent round trips, ~20 us of latency in a 48 us iteration.
template <typename S>
__global__ __launch_bounds__(1024) void step_trace_k(const S* __restrict__ logits, const long long* __restrict__ labels,
                                                     const float* __restrict__ loss, const float* __restrict__ reg,
                                                     const GradGuardBlock* __restrict__ guard,
                                                     const TraceAdamState* __restrict__ adam,
                                                     const TraceBatchState* __restrict__ batch, TraceHead* __restrict__ head,
                                                     unsigned char* __restrict__ ring, unsigned capacity, long long B, int C,
                                                     int P) {
  __shared__ int red[2][16];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, sub = lane & (P - 1);
  const int rows_per_wave = 64 / P;
  // thread 0 fetches the blocks first, so that their round trip runs under the row loop (stream order: the launches
  // that wrote them are over)
  unsigned seq = 0u, present = 0u, w_loss = 0u;
  unsigned w_reg = 0u, w_norm = 0u, w_coef = 0u, w_halted = 0u, w_bad = 0u, w_steps = 0u, w_lr = 0u, w_batches = 0u;
  if (threadIdx.x == 0) {
    seq = head->records_done;
    w_loss = __float_as_uint(loss[0]);
    if (reg) present |= TRACE_HAS_REG, w_reg = __float_as_uint(reg[0]);
    if (guard) {
      present |= TRACE_HAS_GUARD;
      w_norm = __float_as_uint(guard->last_norm), w_coef = __float_as_uint(guard->coef);
      w_halted = guard->halted, w_bad = (unsigned)guard->bad_step;
    }
    if (adam) present |= TRACE_HAS_ADAM, w_steps = (unsigned)adam->steps_done, w_lr = __float_as_uint(adam->lr);
    if (batch) present |= TRACE_HAS_SOURCE, w_batches = batch->batches_done;
  }
  int rows = 0, correct = 0;   // only a row's first lane adds to them
  // (wave-uniform trip count: the shuffles below need every lane of the wave)
  for (long long r0 = (long long)wave * rows_per_wave; r0 < B; r0 += 16LL * rows_per_wave) {
    const long long b = r0 + lane / P;
    const bool live = b < B;
    const S* row = logits + (live ? b : 0) * C;
    const long long y = live && sub == 0 ? labels[b] : TRACE_IGNORE;
    float m = -INFINITY;
    int first = 0x7fffffff;
    for (int c0 = sub; c0 < C; c0 += P * TRACE_UNROLL) {   // (its own trip count per lane: no shuffle inside)
      float v[TRACE_UNROLL];
#pragma unroll
      for (int j = 0; j < TRACE_UNROLL; ++j) {
        const int c = c0 + j * P;
        v[j] = c < C ? tr_ld(row + c) : __builtin_nanf("");
      }
#pragma unroll
      for (int j = 0; j < TRACE_UNROLL; ++j)   // ascending class index
        if (v[j] > m || (first == 0x7fffffff && v[j] == m)) m = v[j], first = c0 + j * P;
    }
    for (int off = P >> 1; off > 0; off >>= 1) {
      const float m2 = __shfl_xor(m, off, 64);
      const int first2 = __shfl_xor(first, off, 64);
      tr_better(m, first, m2, first2);
    }
    if (y != TRACE_IGNORE) {   // (live && sub == 0)
      rows += 1;
      correct += (y >= 0 && y < C && y == (long long)first) ? 1 : 0;
    }
  }
  for (int off = 32; off > 0; off >>= 1) {
    rows += __shfl_down(rows, off, 64);
    correct += __shfl_down(correct, off, 64);
  }
  if (lane == 0) red[0][wave] = rows, red[1][wave] = correct;
  __syncthreads();
  if (threadIdx.x != 0) return;
  int total_rows = 0, total_correct = 0;
  for (int k = 0; k < 16; ++k) total_rows += red[0][k], total_correct += red[1][k];
  // all 64 bytes of the slot, as four 16-byte vector stores (the slot is 16-byte aligned: ring is, and 64 divides by 16);
  // stream order makes the read-modify-write of the head safe: one workgroup, one launch at a time
  uint4* slot = reinterpret_cast<uint4*>(ring + (size_t)(seq % capacity) * TRACE_RECORD_BYTES);
  slot[0] = make_uint4(seq, present, w_loss, w_reg);
  slot[1] = make_uint4((unsigned)total_rows, (unsigned)total_correct, w_norm, w_coef);
  slot[2] = make_uint4(w_halted, w_bad, w_steps, w_lr);
  slot[3] = make_uint4(w_batches, 0u, 0u, 0u);
  head->records_done = seq + 1u;
}

}  // namespace

extern "C" {

size_t dctn_step_trace_head_bytes(void) { return sizeof(TraceHead); }

size_t dctn_step_trace_record_bytes(void) { return TRACE_RECORD_BYTES; }

int dctn_step_trace_record(const void* logits, const void* labels, const void* loss, const void* reg_or_null,
                           const void* guard_or_null, const void* adam_state_or_null, const void* batch_state_or_null,
                           void* head, void* ring, int capacity, int64_t B, int C, int dtype, void* stream) {
  if (!logits || !labels || !loss || !head || !ring) return DCTN_ERR_NULL;
  if (B < 1 || C < 1 || capacity < 1) return DCTN_ERR_BAD_SHAPE;
  if (dtype != DCTN_F32 && dtype != DCTN_BF16) return DCTN_ERR_BAD_DTYPE;
  hipStream_t st = (hipStream_t)stream;
  int P = 1;   // lanes per row: every lane takes up to TRACE_UNROLL classes per round
  while (P * TRACE_UNROLL < C && P < 64) P <<= 1;
#define DCTN_TRACE_LAUNCH(S)                                                                                          \
  hipLaunchKernelGGL(step_trace_k<S>, dim3(1), dim3(1024), 0, st, (const S*)logits, (const long long*)labels,        \
                     (const float*)loss, (const float*)reg_or_null, (const GradGuardBlock*)guard_or_null,             \
                     (const TraceAdamState*)adam_state_or_null, (const TraceBatchState*)batch_state_or_null,          \
                     (TraceHead*)head, (unsigned char*)ring, (unsigned)capacity, (long long)B, C, P)
  if (dtype == DCTN_F32) DCTN_TRACE_LAUNCH(float); else DCTN_TRACE_LAUNCH(bf16_t);
#undef DCTN_TRACE_LAUNCH
  DCTN_CHECK_LAUNCH();
  return DCTN_OK;
}

}  // extern "C"
