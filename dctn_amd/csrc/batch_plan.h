// What travels from the one planner of the batch sources (batch_call.hip) to the three files that hold their kernels:
// the public descriptor of a launch (dctn_batch_call_t, include/dctn_amd.h), the plan made from it, and the ONE place
// where both become the kernels' argument.  batch_source.hip, colour_source.hip and augment_source.hip each define one
// plain function that takes the two and walks its typed launch ladder; none of them checks or plans anything.
#pragma once
#include "draw_order.h"

// Outside the unnamed namespace: it crosses translation units.  Everything in it is decided by batch_plan.
struct BatchPlan {
  bool draw, pad;       // a draw (else a gather); DCTN_BATCH_PAD_TAIL
  unsigned S, bits;     // draw only: batches per epoch (ceil with pad), max(2, bit length of n - 1)
  unsigned wgs;         // workgroups: a wave per sample, at most min(CUs, BATCH_MAX_WGS)
  int channels;         // source channels of a byte source: src_channels of the colour source, 1 for the grey table
  unsigned region;      // augmented draws: bytes of a wave's LDS region (a multiple of 16); the launch's dynamic LDS is
                        // BATCH_WAVES regions
};

void batch_source_launch(const dctn_batch_call_t& c, const BatchPlan& p, hipStream_t st);     // U8_TABLE, ROWS
void colour_source_launch(const dctn_batch_call_t& c, const BatchPlan& p, hipStream_t st);    // COLOUR
void augment_source_launch(const dctn_batch_call_t& c, const BatchPlan& p, hipStream_t st);   // augment != 0

namespace {

constexpr unsigned AUG_WAVE_LDS = 13u * 1024u;   // bytes of one wave's sample region (augment_source.hip)

// A draw leaves sample_idx NULL, a gather the state block and every word of the order zero: no kernel of the other
// operation reads them.
inline BatchArgs batch_args(const dctn_batch_call_t& c, const BatchPlan& p) {
  BatchArgs a = {};
  a.src = c.src, a.table = c.table, a.labels = static_cast<const long long*>(c.labels);
  a.x = c.x, a.y = static_cast<long long*>(c.y), a.indices = static_cast<long long*>(c.indices);
  a.n = (unsigned)c.n, a.Bl = (unsigned)c.count, a.row_len = (unsigned)c.row_len, a.width = (unsigned)c.width;
  if (p.draw) {
    a.state = static_cast<BatchState*>(c.state);
    a.identity = (c.flags & DCTN_BATCH_IDENTITY_ORDER) ? 1u : 0u;
    a.G = (unsigned)c.global_batch, a.S = p.S, a.offset = (unsigned)c.rank_offset, a.bits = p.bits;
  } else {
    a.sample_idx = static_cast<const long long*>(c.sample_idx);
  }
  return a;
}

}  // namespace
