// The host side of every batch-source launch (batch_source.hip, colour_source.hip, augment_source.hip hold the kernels):
// ONE description of a launch (dctn_batch_call_t, include/dctn_amd.h), ONE copy of the checks and of the planning
// (batch_plan), ONE table of the names dctn_last_kernel() reports.  dctn_batch_draw_call / dctn_batch_gather_call take the
// descriptor; the six older entry points only fill it.  No kernel lives here.
#include "batch_plan.h"

namespace {

// Everything is decided here, on the host, before any launch.  The codes come in one order for every kind - NULL, shape,
// dtype, unsupported - with ONE exception that the older entry points had and keep: the source kind is looked at between
// the pointers every launch needs and the table, because only the kind says whether there is a table.  What differs
// between the kinds is written where it differs:
//   ROWS    : no table (it may be NULL), no source channels
//   COLOUR  : src_channels <= width <= src_channels + 1, both at most 4
//   augment : draws of the two byte sources only; of `flags` the identity order only (an evaluation pass is not augmented);
//             row_len = height * width_px; a sample has to fit a wave's LDS region
int batch_plan(const dctn_batch_call_t* call, bool draw, BatchPlan& p) {
  if (!call) return DCTN_ERR_NULL;
  const dctn_batch_call_t& c = *call;
  const bool rows = c.src_kind == DCTN_BATCH_SRC_ROWS, colour = c.src_kind == DCTN_BATCH_SRC_COLOUR, aug = c.augment != 0;
  const int64_t lim = (int64_t)1 << 31;
  if (!c.src || !c.labels || !c.x || !c.y || !c.indices || (draw ? !c.state : !c.sample_idx)) return DCTN_ERR_NULL;
  if (c.src_kind != DCTN_BATCH_SRC_U8_TABLE && !rows && !colour) return DCTN_ERR_BAD_SHAPE;
  if (aug && (!draw || rows)) return DCTN_ERR_BAD_SHAPE;   // no augmented gather; rows have no height and width
  if (!rows && !c.table) return DCTN_ERR_NULL;
  if (c.n < 1 || c.n >= lim || c.count < 1 || c.count >= lim) return DCTN_ERR_BAD_SHAPE;
  if (aug && (c.height < 1 || c.height >= lim || c.width_px < 1 || c.width_px >= lim || c.row_len != c.height * c.width_px))
    return DCTN_ERR_BAD_SHAPE;
  p.channels = colour ? c.src_channels : 1;
  if (c.row_len < 1 || c.row_len >= lim || p.channels < 1 || c.width < 1) return DCTN_ERR_BAD_SHAPE;
  if (draw) {
    if (c.global_batch < 1 || c.global_batch > c.n || c.rank_offset < 0 || c.rank_offset + c.count > c.global_batch)
      return DCTN_ERR_BAD_SHAPE;
    if (c.flags & ~(aug ? DCTN_BATCH_IDENTITY_ORDER : DCTN_BATCH_IDENTITY_ORDER | DCTN_BATCH_PAD_TAIL)) return DCTN_ERR_BAD_SHAPE;
    if ((c.flags & DCTN_BATCH_PAD_TAIL) && !(c.flags & DCTN_BATCH_IDENTITY_ORDER)) return DCTN_ERR_BAD_SHAPE;
  }
  if (aug) {
    if (c.max_shift < 0 || c.max_shift >= 1 << 15 || (c.aug_flags & ~DCTN_AUG_HFLIP)) return DCTN_ERR_BAD_SHAPE;
    if (p.channels < 4 && (c.fill >> (8 * p.channels))) return DCTN_ERR_BAD_SHAPE;   // fill bytes above the source channels
  }
  if (c.dtype != DCTN_F32 && c.dtype != DCTN_F64 && c.dtype != DCTN_BF16) return DCTN_ERR_BAD_DTYPE;
  if (c.width > 4) return DCTN_ERR_UNSUPPORTED;
  if (colour && (p.channels > 4 || c.width < p.channels || c.width > p.channels + 1)) return DCTN_ERR_UNSUPPORTED;
  const int64_t region = aug ? (c.row_len * p.channels + 15) / 16 * 16 : 0;
  if (region > (int64_t)AUG_WAVE_LDS) return DCTN_ERR_UNSUPPORTED;
  p.draw = draw, p.pad = draw && (c.flags & DCTN_BATCH_PAD_TAIL), p.region = (unsigned)region;
  p.S = p.bits = 0;
  if (draw) {
    p.S = (unsigned)(p.pad ? (c.n + c.global_batch - 1) / c.global_batch : c.n / c.global_batch);
    p.bits = 2;
    while (p.bits < 31 && ((int64_t)1 << p.bits) < c.n) ++p.bits;
  }
  long long wgs = (c.count + BATCH_WAVES - 1) / BATCH_WAVES;
  const long long cap = dctn_dev().cus < BATCH_MAX_WGS ? (dctn_dev().cus < 1 ? 1 : dctn_dev().cus) : BATCH_MAX_WGS;
  p.wgs = (unsigned)(wgs > cap ? cap : wgs);
  return DCTN_OK;
}

// [draw / gather][augmented][source kind][dtype code]; there is no augmented gather and no augmented row copy
const char* const BATCH_KERNEL_NAMES[2][2][3][3] = {
    {{{"batch_draw_u8_f32", "batch_draw_u8_f64", "batch_draw_u8_bf16"},
      {"batch_draw_rows_f32", "batch_draw_rows_f64", "batch_draw_rows_bf16"},
      {"colour_draw_f32", "colour_draw_f64", "colour_draw_bf16"}},
     {{"aug_draw_u8_f32", "aug_draw_u8_f64", "aug_draw_u8_bf16"},
      {nullptr, nullptr, nullptr},
      {"aug_draw_cols_f32", "aug_draw_cols_f64", "aug_draw_cols_bf16"}}},
    {{{"batch_gather_u8_f32", "batch_gather_u8_f64", "batch_gather_u8_bf16"},
      {"batch_gather_rows_f32", "batch_gather_rows_f64", "batch_gather_rows_bf16"},
      {"colour_gather_f32", "colour_gather_f64", "colour_gather_bf16"}},
     {{nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr}}},
};

int batch_call(const dctn_batch_call_t* c, bool draw, void* stream) {
  BatchPlan p;
  const int rc = batch_plan(c, draw, p);
  if (rc != DCTN_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (c->augment) augment_source_launch(*c, p, st);
  else if (c->src_kind == DCTN_BATCH_SRC_COLOUR) colour_source_launch(*c, p, st);
  else batch_source_launch(*c, p, st);
  DCTN_CHECK_LAUNCH();
  dctn_set_last_kernel(BATCH_KERNEL_NAMES[draw ? 0 : 1][c->augment ? 1 : 0][c->src_kind][c->dtype]);
  return DCTN_OK;
}

// what the four older draws have in common
dctn_batch_call_t draw_fields(const void* src, const void* table, const void* labels, void* x, void* y, void* indices,
                              void* state, int64_t n, int64_t global_batch, int64_t local_batch, int64_t rank_offset,
                              int src_kind, int width, int flags, int dtype) {
  dctn_batch_call_t c = {};
  c.src = src, c.table = table, c.labels = labels, c.x = x, c.y = y, c.indices = indices, c.state = state;
  c.n = n, c.global_batch = global_batch, c.count = local_batch, c.rank_offset = rank_offset;
  c.src_kind = src_kind, c.width = width, c.flags = flags, c.dtype = dtype;
  return c;
}

dctn_batch_call_t gather_fields(const void* src, const void* table, const void* labels, const void* sample_idx, void* x,
                                void* y, void* indices, int64_t n, int64_t count, int64_t row_len, int src_kind, int width,
                                int dtype) {
  dctn_batch_call_t c = {};
  c.src = src, c.table = table, c.labels = labels, c.sample_idx = sample_idx, c.x = x, c.y = y, c.indices = indices;
  c.n = n, c.count = count, c.row_len = row_len, c.src_kind = src_kind, c.width = width, c.dtype = dtype;
  return c;
}

// the augmented forms give height and width_px in place of row_len (unsigned: a product of bad arguments may wrap, and
// batch_plan refuses them before it looks at it)
void augment_fields(dctn_batch_call_t& c, int64_t height, int64_t width_px, int max_shift, int aug_flags, uint32_t fill) {
  c.height = height, c.width_px = width_px, c.row_len = (int64_t)((uint64_t)height * (uint64_t)width_px);
  c.augment = 1, c.max_shift = max_shift, c.aug_flags = aug_flags, c.fill = fill;
}

// dctn_batch_draw / dctn_batch_gather name two kinds: the colour source has entry points of its own there
int grey_or_rows(int src_kind) { return src_kind == DCTN_BATCH_SRC_COLOUR ? -1 : src_kind; }

}  // namespace

extern "C" {

size_t dctn_batch_state_bytes(void) { return sizeof(BatchState); }
size_t dctn_batch_call_bytes(void) { return sizeof(dctn_batch_call_t); }

int dctn_batch_draw_call(const dctn_batch_call_t* call, void* stream) { return batch_call(call, true, stream); }
int dctn_batch_gather_call(const dctn_batch_call_t* call, void* stream) { return batch_call(call, false, stream); }

int dctn_batch_draw(const void* src, const void* table, const void* labels, void* x, void* y, void* indices, void* state,
                    int64_t n, int64_t global_batch, int64_t local_batch, int64_t rank_offset, int64_t row_len, int width,
                    int src_kind, int flags, int dtype, void* stream) {
  dctn_batch_call_t c = draw_fields(src, table, labels, x, y, indices, state, n, global_batch, local_batch, rank_offset,
                                    grey_or_rows(src_kind), width, flags, dtype);
  c.row_len = row_len;
  return batch_call(&c, true, stream);
}

int dctn_batch_gather(const void* src, const void* table, const void* labels, const void* sample_idx, void* x, void* y,
                      void* indices, int64_t n, int64_t count, int64_t row_len, int width, int src_kind, int dtype,
                      void* stream) {
  const dctn_batch_call_t c = gather_fields(src, table, labels, sample_idx, x, y, indices, n, count, row_len,
                                            grey_or_rows(src_kind), width, dtype);
  return batch_call(&c, false, stream);
}

int dctn_batch_draw_cols(const void* src, const void* table, const void* labels, void* x, void* y, void* indices,
                         void* state, int64_t n, int64_t global_batch, int64_t local_batch, int64_t rank_offset,
                         int64_t pixels, int src_channels, int width, int flags, int dtype, void* stream) {
  dctn_batch_call_t c = draw_fields(src, table, labels, x, y, indices, state, n, global_batch, local_batch, rank_offset,
                                    DCTN_BATCH_SRC_COLOUR, width, flags, dtype);
  c.row_len = pixels, c.src_channels = src_channels;
  return batch_call(&c, true, stream);
}

int dctn_batch_gather_cols(const void* src, const void* table, const void* labels, const void* sample_idx, void* x, void* y,
                           void* indices, int64_t n, int64_t count, int64_t pixels, int src_channels, int width, int dtype,
                           void* stream) {
  dctn_batch_call_t c = gather_fields(src, table, labels, sample_idx, x, y, indices, n, count, pixels,
                                      DCTN_BATCH_SRC_COLOUR, width, dtype);
  c.src_channels = src_channels;
  return batch_call(&c, false, stream);
}

int dctn_batch_draw_aug(const void* src, const void* table, const void* labels, void* x, void* y, void* indices, void* state,
                        int64_t n, int64_t global_batch, int64_t local_batch, int64_t rank_offset, int64_t height,
                        int64_t width_px, int width, int flags, int dtype, int max_shift, int aug_flags, uint32_t fill,
                        void* stream) {
  dctn_batch_call_t c = draw_fields(src, table, labels, x, y, indices, state, n, global_batch, local_batch, rank_offset,
                                    DCTN_BATCH_SRC_U8_TABLE, width, flags, dtype);
  augment_fields(c, height, width_px, max_shift, aug_flags, fill);
  return batch_call(&c, true, stream);
}

int dctn_batch_draw_cols_aug(const void* src, const void* table, const void* labels, void* x, void* y, void* indices,
                             void* state, int64_t n, int64_t global_batch, int64_t local_batch, int64_t rank_offset,
                             int64_t height, int64_t width_px, int src_channels, int width, int flags, int dtype,
                             int max_shift, int aug_flags, uint32_t fill, void* stream) {
  dctn_batch_call_t c = draw_fields(src, table, labels, x, y, indices, state, n, global_batch, local_batch, rank_offset,
                                    DCTN_BATCH_SRC_COLOUR, width, flags, dtype);
  c.src_channels = src_channels;
  augment_fields(c, height, width_px, max_shift, aug_flags, fill);
  return batch_call(&c, true, stream);
}

}  // extern "C"
