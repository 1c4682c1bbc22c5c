// Colour-corrected evaluation (examples/lib_bilagrid.py:56-126 color_correct):
// the render is warped onto the ground truth by a quadratic colour map fitted
// by least squares over the unclipped pixels, a few times over.  The reference
// solves 3 masked [P,10] systems per iteration with torch.linalg.lstsq; the
// same solution needs 65 masked sums per channel (the 55 distinct entries of
// G = sum a a^T and the 10 of h = sum a ref) and a 10 x 10 solve.
//
// Per iteration, three launches and no host read:
//   accumulate  grid (NB, 3): blockIdx.y is the output channel, so a lane
//     holds 65 float64 sums (3 x 65 would not fit the register file).  A lane
//     takes groups of 4 pixels (three 16-byte loads per array), grid-strided;
//     the sums are reduced over the wave (wave_ops.h), over the workgroup's 4
//     waves in wave order and stored as one partial row.  NB depends on P
//     alone and nothing is atomic: the same input gives the same bits.
//   solve       grid 3: a workgroup per channel adds the partial rows in a
//     fixed order, thread 0 scales by the diagonal, runs the Cholesky
//     factorisation with the pivot test and both substitutions, all unrolled
//     in registers, and writes column c of W[10,3] and the fallback flag.
//   warp        a(x) W in float64, clip, one rounding to float32, into `out`
//     (in place from the second iteration on).
#include "wave_ops.h"

namespace gs {
namespace cck {

constexpr int NT = 256;        // lanes per workgroup
constexpr int PX = 4;          // pixels per lane and step: 12 floats = 3 x float4
constexpr int NS = 65;         // sums per channel: 55 of G, 10 of h
constexpr int NF = 10;         // features
// Workgroups per channel at most: 3 x 168 = 504 workgroups of 4 waves are
// resident at once on 256 CUs at 2 waves per SIMD, so every lane runs a long
// loop and the 65 wave reductions are paid once.
constexpr int MAX_NB = 168;
constexpr int SOLVE_Q = 8;     // the solve adds the partial rows in 8 interleaved runs
constexpr double PIVOT_MIN = 1e-10;

inline int64_t groups(int64_t P) { return (P + PX - 1) / PX; }
inline int num_blocks(int64_t P) {
  const int64_t nb = (groups(P) + NT - 1) / NT;
  return (int)std::min<int64_t>(std::max<int64_t>(nb, 1), MAX_NB);
}

// The 12 floats of pixel group g of a [P,3] array; pixels past P read as 0
// (below any eps: masked out of the fit, never stored).
GS_INLINE void load_group(const float *__restrict__ a, int64_t g, int64_t P, float (&v)[3 * PX]) {
  if (g * PX + PX <= P) {
    const float4 *q = reinterpret_cast<const float4 *>(a) + 3 * g;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float4 t = q[k];
      v[4 * k] = t.x, v[4 * k + 1] = t.y, v[4 * k + 2] = t.z, v[4 * k + 3] = t.w;
    }
  } else {
    const int64_t n = 3 * (P - g * PX);  // floats left, 3 .. 9
#pragma unroll
    for (int k = 0; k < 3 * PX; ++k) v[k] = k < n ? a[3 * PX * g + k] : 0.f;
  }
}

// Channel c of pixel j of a group, by selects (a register array has no
// run-time index).
GS_INLINE float pick3(const float (&v)[3 * PX], int j, int c) {
  return c == 0 ? v[3 * j] : c == 1 ? v[3 * j + 1] : v[3 * j + 2];
}

GS_INLINE void features(double x0, double x1, double x2, double (&a)[NF]) {
  a[0] = x0 * x0, a[1] = x0 * x1, a[2] = x0 * x2, a[3] = x1 * x1, a[4] = x1 * x2, a[5] = x2 * x2;
  a[6] = x0, a[7] = x1, a[8] = x2, a[9] = 1.0;
}

// partial[(c * NB + block) * NS + s]: s < 55 the upper triangle of G_c by rows,
// then h_c.
__global__ void __launch_bounds__(NT)
accumulate_kernel(int64_t P, const float *__restrict__ img, const float *__restrict__ x,
                  const float *__restrict__ ref, float lo, float hi,
                  double *__restrict__ partial) {
  __shared__ double red[NT / kWave][NS];
  const int c = blockIdx.y, tid = threadIdx.x;
  const bool first = img == x;  // the first iteration: one mask test fewer, one array fewer
  double acc[NS];
#pragma unroll
  for (int s = 0; s < NS; ++s) acc[s] = 0.0;

  const int64_t G = (P + PX - 1) / PX, stride = (int64_t)gridDim.x * NT;
  for (int64_t g = (int64_t)blockIdx.x * NT + tid; g < G; g += stride) {
    float xv[3 * PX], rv[3 * PX], iv[3 * PX];
    load_group(x, g, P, xv);
    load_group(ref, g, P, rv);
    if (!first) load_group(img, g, P, iv);
#pragma unroll
    for (int j = 0; j < PX; ++j) {
      const float xc = pick3(xv, j, c), rc = pick3(rv, j, c);
      const float ic = first ? xc : pick3(iv, j, c);
      const bool m = ic >= lo && ic <= hi && xc >= lo && xc <= hi && rc >= lo && rc <= hi;
      if (m) {
        double a[NF];
        features((double)xv[3 * j], (double)xv[3 * j + 1], (double)xv[3 * j + 2], a);
        int s = 0;
#pragma unroll
        for (int r = 0; r < NF; ++r)
#pragma unroll
          for (int q = r; q < NF; ++q) acc[s] = fma(a[r], a[q], acc[s]), ++s;
        const double b = (double)rc;
#pragma unroll
        for (int r = 0; r < NF; ++r) acc[55 + r] = fma(a[r], b, acc[55 + r]);
      }
    }
  }

  const int wave = tid / kWave, lane = tid % kWave;
#pragma unroll
  for (int s = 0; s < NS; ++s) {
    const double t = wave_sum(acc[s]);
    if (lane == 0) red[wave][s] = t;
  }
  __syncthreads();
  if (tid < NS) {
    double t = red[0][tid];
#pragma unroll
    for (int w = 1; w < NT / kWave; ++w) t += red[w][tid];
    partial[((int64_t)c * gridDim.x + blockIdx.x) * NS + tid] = t;
  }
}

// Upper-triangle index of (r, q), r <= q, rows of length 10, 9, ...
constexpr int tri(int r, int q) { return r * NF - r * (r - 1) / 2 + (q - r); }

__global__ void __launch_bounds__(SOLVE_Q *NS)
solve_kernel(int nb, const double *__restrict__ partial, double *__restrict__ W,
             int32_t *__restrict__ fallback) {
  __shared__ double red[SOLVE_Q][NS];
  __shared__ double tot[NS];
  const int c = blockIdx.x, tid = threadIdx.x;
  {
    const int s = tid % NS, q = tid / NS;
    const double *row = partial + (int64_t)c * nb * NS + s;
    double t = 0.0;
#pragma unroll 8
    for (int b = q; b < nb; b += SOLVE_Q) t += row[(int64_t)b * NS];
    red[q][s] = t;
  }
  __syncthreads();
  if (tid < NS) {
    double t = red[0][tid];
#pragma unroll
    for (int q = 1; q < SOLVE_Q; ++q) t += red[q][tid];
    tot[tid] = t;
  }
  __syncthreads();
  if (tid != 0) return;

  // G' = D^-1/2 G D^-1/2 (unit diagonal), factored in place: L[tri(r, q)] is
  // L(q, r), the upper triangle of L^T.
  double L[55], is[NF], y[NF];
  bool ok = tot[tri(9, 9)] >= 10.0;  // the rows of the fit: the sum of 1 * 1
#pragma unroll
  for (int r = 0; r < NF; ++r) {
    const double d = tot[tri(r, r)];
    ok = ok && d > 0.0;
    is[r] = d > 0.0 ? 1.0 / sqrt(d) : 0.0;
  }
#pragma unroll
  for (int r = 0; r < NF; ++r)
#pragma unroll
    for (int q = r; q < NF; ++q) L[tri(r, q)] = tot[tri(r, q)] * is[r] * is[q];
#pragma unroll
  for (int r = 0; r < NF; ++r) y[r] = tot[55 + r] * is[r];

#pragma unroll
  for (int j = 0; j < NF; ++j) {
    double p = L[tri(j, j)];
#pragma unroll
    for (int k = 0; k < j; ++k) p -= L[tri(k, j)] * L[tri(k, j)];
    ok = ok && p >= PIVOT_MIN;  // false for a NaN too
    const double ljj = sqrt(ok ? p : 1.0), inv = 1.0 / ljj;
    L[tri(j, j)] = ljj;
#pragma unroll
    for (int i = j + 1; i < NF; ++i) {
      double t = L[tri(j, i)];
#pragma unroll
      for (int k = 0; k < j; ++k) t -= L[tri(k, i)] * L[tri(k, j)];
      L[tri(j, i)] = t * inv;
    }
  }
  // L y' = y, then L^T z = y'
#pragma unroll
  for (int i = 0; i < NF; ++i) {
    double t = y[i];
#pragma unroll
    for (int k = 0; k < i; ++k) t -= L[tri(k, i)] * y[k];
    y[i] = t / L[tri(i, i)];
  }
#pragma unroll
  for (int i = NF - 1; i >= 0; --i) {
    double t = y[i];
#pragma unroll
    for (int k = i + 1; k < NF; ++k) t -= L[tri(i, k)] * y[k];
    y[i] = t / L[tri(i, i)];
  }
#pragma unroll
  for (int r = 0; r < NF; ++r) W[r * 3 + c] = ok ? y[r] * is[r] : (r == 6 + c ? 1.0 : 0.0);
  if (fallback) fallback[c] = ok ? 0 : 1;
}

__global__ void __launch_bounds__(NT)
warp_kernel(int64_t P, const float *x, const double *__restrict__ W, float *out) {
  // x == out from the second iteration on: a lane reads its group, then stores it
  const int64_t g = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (g * PX >= P) return;
  double w[NF * 3];
#pragma unroll
  for (int k = 0; k < NF * 3; ++k) w[k] = W[k];
  float xv[3 * PX], ov[3 * PX];
  load_group(x, g, P, xv);
#pragma unroll
  for (int j = 0; j < PX; ++j) {
    double a[NF];
    features((double)xv[3 * j], (double)xv[3 * j + 1], (double)xv[3 * j + 2], a);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      double t = 0.0;
#pragma unroll
      for (int r = 0; r < NF; ++r) t = fma(a[r], w[r * 3 + c], t);
      ov[3 * j + c] = (float)fmin(fmax(t, 0.0), 1.0);
    }
  }
  if (g * PX + PX <= P) {
    float4 *q = reinterpret_cast<float4 *>(out) + 3 * g;
#pragma unroll
    for (int k = 0; k < 3; ++k)
      q[k] = make_float4(ov[4 * k], ov[4 * k + 1], ov[4 * k + 2], ov[4 * k + 3]);
  } else {
    const int64_t n = 3 * (P - g * PX);
#pragma unroll
    for (int k = 0; k < 3 * PX; ++k)
      if (k < n) out[3 * PX * g + k] = ov[k];
  }
}

inline int64_t partial_bytes(int64_t P) { return (int64_t)3 * num_blocks(P) * NS * 8; }

}  // namespace cck
}  // namespace gs

using namespace gs;

// the partial rows, then W[10,3]
extern "C" int64_t gsplat_hip_color_correct_workspace_bytes(int64_t P) {
  if (P < 1) return 0;
  return cck::partial_bytes(P) + cck::NF * 3 * 8;
}

extern "C" int gsplat_hip_color_correct(int64_t P, const float *img, const float *ref,
                                        int num_iters, double eps, float *out, void *workspace,
                                        int32_t *fallbacks, void *stream) {
  GS_REQUIRE(P >= 1 && P < ((int64_t)1 << 40), "color_correct: P %lld outside [1, 2^40)",
             (long long)P);
  GS_REQUIRE(num_iters >= 0, "color_correct: num_iters %d < 0", num_iters);
  GS_REQUIRE(eps > 0.0 && eps < 0.5, "color_correct: eps %g outside (0, 0.5)", eps);
  GS_REQUIRE(img && ref && out && workspace, "color_correct: null pointer");
  GS_REQUIRE((((uintptr_t)img | (uintptr_t)ref | (uintptr_t)out | (uintptr_t)workspace) & 15) == 0,
             "color_correct: img, ref, out and workspace must be 16-B aligned");
  const uintptr_t bytes = (uintptr_t)P * 12;
  GS_REQUIRE((uintptr_t)out + bytes <= (uintptr_t)img || (uintptr_t)img + bytes <= (uintptr_t)out,
             "color_correct: out must not overlap img");
  hipStream_t st = (hipStream_t)stream;
  if (num_iters == 0) {
    GS_HIP(hipMemcpyAsync(out, img, bytes, hipMemcpyDeviceToDevice, st));
    return 0;
  }
  const int nb = cck::num_blocks(P);
  double *partial = reinterpret_cast<double *>(workspace);
  double *W = reinterpret_cast<double *>(reinterpret_cast<char *>(workspace) +
                                         cck::partial_bytes(P));
  const float lo = (float)eps, hi = (float)(1.0 - eps);
  const unsigned wg = (unsigned)((cck::groups(P) + cck::NT - 1) / cck::NT);
  for (int it = 0; it < num_iters; ++it) {
    const float *x = it == 0 ? img : out;
    hipLaunchKernelGGL(cck::accumulate_kernel, dim3((unsigned)nb, 3), dim3(cck::NT), 0, st, P, img,
                       x, ref, lo, hi, partial);
    hipLaunchKernelGGL(cck::solve_kernel, dim3(3), dim3(cck::SOLVE_Q * cck::NS), 0, st, nb,
                       partial, W, fallbacks ? fallbacks + 3 * it : nullptr);
    hipLaunchKernelGGL(cck::warp_kernel, dim3(wg), dim3(cck::NT), 0, st, P, x, W, out);
  }
  GS_CHECK_LAUNCH("color_correct");
  return 0;
}
