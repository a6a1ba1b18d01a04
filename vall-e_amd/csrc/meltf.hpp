// Launcher of the mel-Transformer decode step's opening kernel (meltf.hip, a translation unit of its own).
#pragma once
#include "common.hpp"

namespace vx {

constexpr int MEL_BINS = 100;      // NUM_MEL_BINS, valle/models/macros.py
constexpr int MEL_HEAD = 101;      // predict_layer's 100 rows, then stop_layer's one
constexpr int MEL_PRENET_H = 256;  // hidden width of the MLP decoder prenet (models/transformer.py:87-95)
constexpr int MEL_GRID = 16;      // workgroups of the step's opening kernel: 16 x 64 rows cover d <= 1024

// Device-resident words of the step besides ArState (which carries S, row, pass, n_gen, done and stop_reason as in the token
// models; row == -1 is "nothing processed yet": the first launch only forms input row 0 from the all-zero frame).
struct MelCtl {
  unsigned arrive;      // workgroups that have read the state in this launch; the one that arrives last does the book-keeping
  int max_frames;       // engine-level limit on appended frames
  int n_forced;         // > 0: teacher forcing - the fed-back frame of pass p is forced[p], the decode ends after n_forced passes
  int pad;
  const float* forced;  // (n_forced, MEL_BINS)
};

struct MelStepArgs {
  const float* xh;             // (d) residual row the last layer left for the head
  const float *gamma, *beta;   // the norm in front of the head: decoder.norm, or the last layer's norm3 of a post-norm stack
  const float *Wh, *bh;        // (MEL_HEAD, d), (MEL_HEAD)
  const float *W1, *b1;        // MLP prenet: (256, 100); null for the linear prenet
  const float *W2, *b2;        // (256, 256)
  const float *W0, *b0;        // the prenet's last (or only) layer: (d, K0), K0 = 256 with the MLP, else 100
  const float *alpha, *pe;     // decoder_position
  float* x;                    // (d) the next input row
  ArState* st;
  MelCtl* ctl;
  float* frames;               // (capacity, MEL_BINS)
  float* stops;                // one stop logit per pass
  int d;
};

__attribute__((visibility("hidden"))) void launch_mel_open(const MelStepArgs& a, hipStream_t s);

}  // namespace vx
