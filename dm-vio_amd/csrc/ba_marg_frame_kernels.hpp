// CDNA4 (gfx950) kernel of the batched FRAME marginalisation: EnergyFunctional::marginalizeFrame, visual-only branch (EnergyFunctional.cpp:570-640), for W windows per
// launch — BAHost::marginalizeFrame (ba_host.hpp) operation for operation, one workgroup per window, the whole problem in LDS.
//
// Why the bits equal the host's: every output element is a fixed-order expression of its inputs (the sums over the frame's 8 unknowns start from 0.0 and run k = 0..7,
// nothing is reduced across threads), the library is built with -ffp-contract=off for host and device alike, and sqrt / division of doubles are correctly rounded on both.
// So no FMA, no reciprocal in place of a division and no other association may be introduced here: the thread mapping is free, the expressions are not.
//
// A window's record in the uploaded slab (doubles, at a fixed stride: baMargFrameInDoubles of the call's largest n):
//   [HM n x n row-major | bM n | prior 8 | delta_prior 8 | ... | (int) F, (int) frame in the stride's last double]       n = 4 + 8 F
// and its result in the downloaded one: [HM_new (n-8) x (n-8) row-major | bM_new n-8].  The records of a launch are consecutive and of one keyframe count (the launch's
// LDS size); both slabs arrive as kernel arguments, so every access to them is a global_load / global_store — no pointer is read from a table.
#pragma once
#include <hip/hip_runtime.h>

namespace dmv {

enum { BA_MARGF_THREADS = 256 };
// row stride of the n x n tile in LDS: n is even, n + 1 doubles keep a column walk (the transposed operand of the last step) off a single pair of banks
__host__ __device__ inline int baMargFrameLd(const int n) { return n + 1; }
// LDS of one workgroup in doubles: [H n x ld | b n | sv n | svi n | A 8 x 16 | bli (n-8) x 8]
__host__ __device__ inline size_t baMargFrameLdsDoubles(const int n) { return (size_t)n * baMargFrameLd(n) + 3 * (size_t)n + 8 * 16 + (size_t)(n - 8) * 8; }
// where a record's members lie (offsets in doubles)
__host__ __device__ inline size_t baMargFrameInDoubles(const int n) { return (size_t)n * n + n + 8 + 8 + 1; }
__host__ __device__ inline size_t baMargFrameOutDoubles(const int n) { return (size_t)(n - 8) * (n - 8) + (n - 8); }

__global__ void __launch_bounds__(BA_MARGF_THREADS) k_ba_marg_frame_b(const double* __restrict__ in, double* __restrict__ out, const size_t inStride, const size_t outStride,
                                                                     const int w0) {
  extern __shared__ double margf_lds[];
  const int tid = threadIdx.x;
  const size_t w = (size_t)w0 + blockIdx.x;
  const double* const rec = in + inStride * w;
  double* const res = out + outStride * w;
  const int* const hdr = reinterpret_cast<const int*>(rec + inStride - 1);   // (F, frame): the stride's last double, wherever the window's own n puts the rest
  const int F = hdr[0], frame = hdr[1];
  const int n = 4 + 8 * F, nd = n - 8, io = 4 + 8 * frame, ld = baMargFrameLd(n);
  const double* const HMg = rec;
  const double* const bMg = rec + (size_t)n * n;
  const double* const prior = bMg + n;
  const double* const dprior = prior + 8;
  double* const H = margf_lds;
  double* const b = H + (size_t)n * ld;
  double* const sv = b + n;
  double* const svi = sv + n;
  double* const A = svi + n;          // 8 x 16: [A | I] -> [I | A^-1]
  double* const bli = A + 8 * 16;     // (n-8) x 8

  // ---- 1. the permuted system (the frame's block moved last), straight from the uploaded prior
  for (int idx = tid; idx < n * n; idx += BA_MARGF_THREADS) {
    const int i = idx / n, j = idx - i * n;
    const int pi = i < io ? i : (i < nd ? i + 8 : i - nd + io);
    const int pj = j < io ? j : (j < nd ? j + 8 : j - nd + io);
    H[i * ld + j] = HMg[(size_t)pi * n + pj];
  }
  for (int i = tid; i < n; i += BA_MARGF_THREADS) b[i] = bMg[i < io ? i : (i < nd ? i + 8 : i - nd + io)];
  __syncthreads();
  if (tid < 8) {
    const double p = prior[tid];
    H[(nd + tid) * ld + nd + tid] += p;
    b[nd + tid] += p * dprior[tid];
  }
  __syncthreads();
  // ---- 2. the diagonal scaling
  for (int i = tid; i < n; i += BA_MARGF_THREADS) { const double s = sqrt(fabs(H[i * ld + i]) + 10); sv[i] = s; svi[i] = 1.0 / s; }
  __syncthreads();
  // ---- 3. (svi_i H_ij) svi_j, svi_i b_i
  for (int idx = tid; idx < n * n; idx += BA_MARGF_THREADS) {
    const int i = idx / n, j = idx - i * n;
    H[i * ld + j] = svi[i] * H[i * ld + j] * svi[j];
  }
  for (int i = tid; i < n; i += BA_MARGF_THREADS) b[i] *= svi[i];
  __syncthreads();
  // ---- 4. the frame block's inverse: Gauss-Jordan on [A | I], one lane per column; the pivot row is found by every thread from the same LDS values (uniform)
  if (tid < 128) {
    const int i = tid >> 4, j = tid & 15;
    A[tid] = j < 8 ? H[(nd + i) * ld + nd + j] : (i == j - 8 ? 1.0 : 0.0);
  }
  __syncthreads();
  for (int c = 0; c < 8; c++) {
    int piv = c;
    double best = fabs(A[c * 16 + c]);
    for (int r = c + 1; r < 8; r++) { const double v = fabs(A[r * 16 + c]); if (v > best) { best = v; piv = r; } }   // the first row with the strictly largest |A[r][c]|
    __syncthreads();
    if (tid < 16 && piv != c) { const double t = A[c * 16 + tid]; A[c * 16 + tid] = A[piv * 16 + tid]; A[piv * 16 + tid] = t; }
    __syncthreads();
    const double d = A[c * 16 + c];
    double m[8];
#pragma unroll
    for (int r = 0; r < 8; r++) m[r] = A[r * 16 + c];
    __syncthreads();
    if (tid < 16) {
      const double x = A[c * 16 + tid] / d;
      A[c * 16 + tid] = x;
#pragma unroll
      for (int r = 0; r < 8; r++) if (r != c && m[r] != 0) A[r * 16 + tid] -= m[r] * x;
    }
    __syncthreads();
  }
  // ---- 5. bli = H_off^T A^-1
  for (int idx = tid; idx < nd * 8; idx += BA_MARGF_THREADS) {
    const int i = idx >> 3, j = idx & 7;
    double s = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) s += H[(nd + k) * ld + i] * A[k * 16 + 8 + j];
    bli[idx] = s;
  }
  __syncthreads();
  // ---- 6. the rank-8 update of the kept part (reads the frame's rows and bli, writes rows above them)
  for (int idx = tid; idx < nd * nd; idx += BA_MARGF_THREADS) {
    const int i = idx / nd, j = idx - i * nd;
    double s = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) s += bli[i * 8 + k] * H[(nd + k) * ld + j];
    H[i * ld + j] -= s;
  }
  for (int i = tid; i < nd; i += BA_MARGF_THREADS) {
    double s = 0;
#pragma unroll
    for (int k = 0; k < 8; k++) s += bli[i * 8 + k] * b[nd + k];
    b[i] -= s;
  }
  __syncthreads();
  // ---- 7. un-scaled and symmetrised
  for (int idx = tid; idx < nd * nd; idx += BA_MARGF_THREADS) {
    const int i = idx / nd, j = idx - i * nd;
    res[idx] = 0.5 * (sv[i] * H[i * ld + j] * sv[j] + sv[j] * H[j * ld + i] * sv[i]);
  }
  for (int i = tid; i < nd; i += BA_MARGF_THREADS) res[(size_t)nd * nd + i] = sv[i] * b[i];
}

}  // namespace dmv
