// Launchers of the text-alignment kernels (align.hip, a translation unit of its own: the device code of every other path is
// compiled without these kernels in sight and stays what it was).
#pragma once
#include "common.hpp"

namespace vx {

constexpr int ALIGN_TILE_ROWS = 32;   // query rows of one workgroup of attn_text_rows_kernel
constexpr int ALIGN_COL_CHUNK = 256;  // text columns one workgroup accumulates; wider windows go over blockIdx.y
constexpr int ALIGN_MAX_SW = 4096;    // widest map mono_path_kernel takes: two fp64 rows of the dynamic programme in 64 KB of LDS

// One attention tap: the head-weighted softmax probabilities the query rows put on the text columns [c0, c1).
//   q      rows x (row stride ldq): head h of row i at q[i * ldq + h * hd + c]
//   k      key j of head h at k[j * ldk + h * k_head_stride + c]  (packed M x 3d rows: ldk = 3 d, k_head_stride = hd;
//          the memory layout (nhead, max_text, hd): ldk = hd, k_head_stride = max_text * hd)
//   causal 1: row i sees keys [0, text_len + row0 + i + 1) - all text keys and the audio keys up to its own (row0: the audio
//          index of row 0); 0: every row sees keys [0, text_len) (the cross-attention memory)
//   head_w nhead weights (device); a zero-weight head is skipped unless per_head is given
//   attn   (rows, c1 - c0) fp32: += sum_h w[h] p_h[i, c] (first != 0: =);  mass (rows) or null: += sum_h w[h] sum_{c < text_len} p_h[i, c]
//   per_head null or (nhead, rows, c1 - c0) fp32: p_h itself, every head
// Returns 0, or -1 for a head size other than 4 / 8 / 16 / 32 / 64.
__attribute__((visibility("hidden"))) int launch_attn_text_rows(bool bf, const void* q, long long ldq, const void* k, long long ldk,
                                                                long long k_head_stride, int rows, int row0, int nhead, int hd,
                                                                int text_len, int causal, int c0, int c1, const float* head_w,
                                                                float* attn, float* mass, float* per_head, int first, hipStream_t s);

// Best monotonic path through the (T, Sw) map a (fp32, row-major): j(0) = 0, j(T-1) = Sw - 1, steps of 0 or 1, maximal
// sum_t log(max(a[t, j(t)], FLT_MIN)) in fp64; on equal predecessors the path stays in its column.  bp: T * Sw bytes of scratch.
// T < Sw: path = -1 everywhere, score = -inf.  Sw <= ALIGN_MAX_SW (the caller checks).
__attribute__((visibility("hidden"))) void launch_mono_path(const float* a, int T, int Sw, unsigned char* bp, int* path, double* score,
                                                            hipStream_t s);

// ---- the batched tap (vx_align_batch): the same quantities over a concatenation of utterances, on the matrix pipe.
constexpr int ALIGN_SEG_ROWS = 64;  // query rows of one workgroup of attn_text_seg_kernel (two waves of 32)

// One utterance (segment) of a batched tap, in a device array.  Its rows are [start, ...) of the packed (M, 3 d) q / k rows (the
// segmented layout: start is a multiple of 64); key j of the segment is row start + j, the first text_len keys are the text.
struct AlignSeg {
  int start;      // first row of the segment
  int text_len;   // text keys
  int qfirst;     // index within the segment of the first tapped row
  int rows;       // tapped rows T_z
  int row0;       // audio index of the first tapped row: tapped row i sees keys [0, text_len + row0 + i + 1)
  int c0, c1;     // text window
  int pad_;
  long long cell_off, row_off;  // where the segment's (T_z, c1 - c0) cells / T_z rows start in the packed outputs
};

// Floats of scratch a batched tap needs: every head's own un-weighted cells and row masses.
inline size_t align_seg_scratch(int nhead, long long cells, long long rows) { return (size_t)nhead * (size_t)(cells + rows); }

// attn_text_seg_kernel + attn_text_heads_kernel: bf16 operands, head_dim 64.  q / k: row i, head h at q[i * ld + h * 64 + c] (the
// packed rows: k = q + d, ld = 3 d).  segs: nseg descriptors (device); max_rows: the largest T_z.  head_w: nhead weights (device);
// a zero-weight head is not computed.  scr: align_seg_scratch(nhead, cells, rows_total) floats, cells / rows_total the extents of
// the packed outputs.  attn (cells) and mass (rows_total, or null): = (first) or += sum_h w[h] p_h, heads added in head order.
__attribute__((visibility("hidden"))) void launch_attn_text_segs(const void* q, const void* k, long long ld, const AlignSeg* segs, int nseg,
                                                                 int max_rows, int nhead, const float* head_w, float* scr,
                                                                 long long cells, long long rows_total, float* attn, float* mass,
                                                                 int first, hipStream_t s);

// mono_path_kernel for n maps at once, one workgroup each: map z is the (rows, c1 - c0) cells at a + segs[z].cell_off, its
// back-pointers at bp + cell_off, its path at path + row_off, its score at score[z].  max_sw: the widest map (<= ALIGN_MAX_SW).
__attribute__((visibility("hidden"))) void launch_mono_path_segs(const float* a, const AlignSeg* segs, int n, int max_sw, unsigned char* bp,
                                                                 int* path, double* score, hipStream_t s);

}  // namespace vx
