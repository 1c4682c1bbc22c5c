// Similarity transforms of splat scenes: x' = A x + t with A = s R per segment.
//   means'  = A means + t          quats' = q_R (x) quats (wxyz, norm kept)
//   scales' = scales + log s       shN'   : per degree l and colour channel the
//   2l+1 coefficients times M_l(R), sum_k a'_k Y_k(d) = sum_k a_k Y_k(R^T d)
//   in the basis of sh_basis.h.
//
// Two kernels, no host read between them:
//   prepare  one lane per segment, float64: s = cbrt(det A), the two validity
//     tests into status[], R = the polar factor of A / s (three Newton-Schulz
//     steps: the deviation allowed is 1e-4, each step squares it), q_R by
//     Shepperd's four-way choice, log s, and the blocks
//     M_l = Y_l(P_l)^-1 Y_l(P_l R) from the directions and inverse matrices of
//     sh_rot_table.h (tools/gen_sh_rot_table.py).  One float32 record per
//     segment: A[9], t[3], q_R[4], log s, s, 2 unused, then M_1..M_L row-major.
//   apply    a workgroup of 128 lanes owns 128 consecutive Gaussians.  Their
//     means, scales and shN rows are contiguous in memory: the workgroup reads
//     them with 16-byte loads into LDS (row stride padded to an odd word count,
//     so a lane walking its own row meets no bank conflict), each lane moves
//     its own row in LDS, and the tile is written back with 16-byte stores.
//     The quaternion is one float4 per lane.  A workgroup reads all of its rows
//     before it writes any and touches no other rows, so outputs may be the
//     inputs.  Without ids the record address is wave-uniform (scalar loads);
//     with ids each lane gathers its segment's record.  A row whose id is
//     outside [0, S), or whose segment's status is nonzero, is copied through;
//     such ids are counted, one integer add per wave that has any.  The data
//     path has no atomics and a fixed operation order: same bits every run.
#include "common.h"
#include "sh_rot_table.h"

namespace gs {
namespace xf {

constexpr int HDR = 20;   // floats in front of the blocks
constexpr int NT = 128;   // lanes, and Gaussians, per workgroup of the apply kernel
constexpr double SIM_TOL = 1e-4;

__host__ __device__ constexpr int block_floats(int deg) {
  return deg <= 0 ? 0 : deg == 1 ? 9 : deg == 2 ? 34 : deg == 3 ? 83 : 164;
}
__host__ __device__ constexpr int record_floats(int deg) { return HDR + block_floats(deg); }
__host__ __device__ constexpr int sh_words(int deg) { return 3 * ((deg + 1) * (deg + 1) - 1); }

// ------------------------------------------------------------------ prepare
// Band L of the basis of sh_basis.h in float64 (sh_basis<> is float and stays
// as the colour kernels have it).
template <int L>
GS_INLINE void basis_band(double x, double y, double z, double *B) {
  const double zz = z * z;
  const double g2 = 2.0 * x * y, h2 = x * x - y * y;
  const double g3 = x * g2 + y * h2, h3 = x * h2 - y * g2;
  if (L == 1) {
    const double C1 = 0.4886025119029199;
    B[0] = -C1 * y, B[1] = C1 * z, B[2] = -C1 * x;
  } else if (L == 2) {
    const double C22 = 0.5462742152960396;
    const double c21 = -1.0925484305920792 * z;
    B[0] = C22 * g2;
    B[1] = c21 * y;
    B[2] = 0.9461746957575601 * zz - 0.3153915652525201;
    B[3] = c21 * x;
    B[4] = C22 * h2;
  } else if (L == 3) {
    const double C33 = -0.5900435899266435, C32 = 1.445305721320277;
    const double c31 = -2.285228997322329 * zz + 0.4570457994644658;
    B[0] = C33 * g3;
    B[1] = C32 * g2 * z;
    B[2] = c31 * y;
    B[3] = z * (1.865881662950577 * zz - 1.119528997770346);
    B[4] = c31 * x;
    B[5] = C32 * h2 * z;
    B[6] = C33 * h3;
  } else {
    const double g4 = x * g3 + y * h3, h4 = x * h3 - y * g3;
    const double C44 = 0.6258357354491761, C43 = -1.7701307697799304;
    const double c41 = z * (-4.683325804901024 * zz + 2.0071396306718676);
    const double c42 = 3.31161143515146 * zz - 0.47308734787878;
    B[0] = C44 * g4;
    B[1] = C43 * g3 * z;
    B[2] = c42 * g2;
    B[3] = c41 * y;
    B[4] = zz * (3.7024941420321507 * zz - 3.1735664074561294) + 0.31735664074561293;
    B[5] = c41 * x;
    B[6] = c42 * h2;
    B[7] = C43 * h3 * z;
    B[8] = C44 * h4;
  }
}

// out[a * n + b] = sum_i YINV[a][i] Y_{L,b}(R^T p_i), rounded to float once.
template <int L>
GS_INLINE void emit_block(const double (&R)[3][3], const double *P, const double *YINV,
                          float *out) {
  constexpr int n = 2 * L + 1;
  double Yr[n][n];
  for (int i = 0; i < n; ++i) {
    const double px = P[3 * i], py = P[3 * i + 1], pz = P[3 * i + 2];
    basis_band<L>(px * R[0][0] + py * R[1][0] + pz * R[2][0],
                  px * R[0][1] + py * R[1][1] + pz * R[2][1],
                  px * R[0][2] + py * R[1][2] + pz * R[2][2], Yr[i]);
  }
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) {
      double acc = 0.0;
      for (int i = 0; i < n; ++i) acc += YINV[a * n + i] * Yr[i][b];
      out[a * n + b] = (float)acc;
    }
}

template <int DEG>
__global__ void __launch_bounds__(64)
prepare_kernel(int64_t S, const double *__restrict__ T, float *__restrict__ rec,
               int32_t *__restrict__ status) {
  const int64_t seg = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (seg >= S) return;
  const double *t = T + (size_t)seg * 16;
  double A[3][3], R[3][3];
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) A[i][j] = t[4 * i + j];
  const double det = A[0][0] * (A[1][1] * A[2][2] - A[1][2] * A[2][1]) -
                     A[0][1] * (A[1][0] * A[2][2] - A[1][2] * A[2][0]) +
                     A[0][2] * (A[1][0] * A[2][1] - A[1][1] * A[2][0]);
  int st = det > 0.0 ? 0 : 1;   // NaN counts as a refusal
  const double s = st ? 1.0 : cbrt(det);
  double dev = 0.0;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      const double g = (A[0][i] * A[0][j] + A[1][i] * A[1][j] + A[2][i] * A[2][j]) / (s * s) -
                       (i == j ? 1.0 : 0.0);
      dev = (fabs(g) > dev || g != g) ? fabs(g) : dev;   // the maximum; a NaN, once in, stays
    }
  if (!(dev <= SIM_TOL)) st |= 2;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) R[i][j] = st ? (i == j ? 1.0 : 0.0) : A[i][j] / s;
  // polar factor: X <- X (3 I - X^T X) / 2
  for (int it = 0; it < 3; ++it) {
    double G[3][3], X[3][3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        G[i][j] = (i == j ? 1.5 : 0.0) -
                  0.5 * (R[0][i] * R[0][j] + R[1][i] * R[1][j] + R[2][i] * R[2][j]);
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        X[i][j] = R[i][0] * G[0][j] + R[i][1] * G[1][j] + R[i][2] * G[2][j];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j) R[i][j] = X[i][j];
  }
  // Shepperd: the largest of tr, R00, R11, R22 picks the formula
  const double tr = R[0][0] + R[1][1] + R[2][2];
  const double a = R[2][1] - R[1][2], b = R[0][2] - R[2][0], c = R[1][0] - R[0][1];
  const double d = R[0][1] + R[1][0], e = R[0][2] + R[2][0], f = R[1][2] + R[2][1];
  double q[4];
  if (tr >= R[0][0] && tr >= R[1][1] && tr >= R[2][2]) {
    q[0] = 1.0 + tr, q[1] = a, q[2] = b, q[3] = c;
  } else if (R[0][0] >= R[1][1] && R[0][0] >= R[2][2]) {
    q[0] = a, q[1] = 1.0 + 2.0 * R[0][0] - tr, q[2] = d, q[3] = e;
  } else if (R[1][1] >= R[2][2]) {
    q[0] = b, q[1] = d, q[2] = 1.0 + 2.0 * R[1][1] - tr, q[3] = f;
  } else {
    q[0] = c, q[1] = e, q[2] = f, q[3] = 1.0 + 2.0 * R[2][2] - tr;
  }
  const double qn = 1.0 / sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);

  float *r = rec + (size_t)seg * record_floats(DEG);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) r[3 * i + j] = (float)A[i][j];
    r[9 + i] = (float)t[4 * i + 3];
  }
#pragma unroll
  for (int i = 0; i < 4; ++i) r[12 + i] = (float)(q[i] * qn);
  r[16] = (float)log(s);
  r[17] = (float)s;
  r[18] = r[19] = 0.f;
  status[seg] = st;
  if (DEG >= 1) emit_block<1>(R, shrot::P1, shrot::YINV1, r + HDR);
  if (DEG >= 2) emit_block<2>(R, shrot::P2, shrot::YINV2, r + HDR + 9);
  if (DEG >= 3) emit_block<3>(R, shrot::P3, shrot::YINV3, r + HDR + 34);
  if (DEG >= 4) emit_block<4>(R, shrot::P4, shrot::YINV4, r + HDR + 83);
}

// -------------------------------------------------------------------- apply
// `rows` rows of W floats starting at row0 (a multiple of NT, so the tile
// starts on a 16-byte boundary of a 16-byte aligned array) <-> LDS rows of WP.
template <int W, int WP>
GS_INLINE void stage_in(const float *g, size_t row0, int rows, float *lds) {
  const float *src = g + row0 * W;
  const float4 *s4 = reinterpret_cast<const float4 *>(src);
  if (rows == NT) {
    // a whole tile: every load of the lane is issued before the first LDS
    // write, so a wave has IT KiB in flight instead of one
    constexpr int NV = NT * W / 4, IT = (NV + NT - 1) / NT;
    float4 x[IT];
#pragma unroll
    for (int k = 0; k < IT; ++k) {
      const int v = k * NT + threadIdx.x;
      if (v < NV) x[k] = s4[v];
    }
#pragma unroll
    for (int k = 0; k < IT; ++k) {
      const int v = k * NT + threadIdx.x;
      if (v < NV) {
        const float xs[4] = {x[k].x, x[k].y, x[k].z, x[k].w};
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const int el = 4 * v + j;
          lds[(el / W) * WP + el % W] = xs[j];
        }
      }
    }
    return;
  }
  const int n = rows * W, nv = n >> 2;
  for (int v = threadIdx.x; v < nv; v += NT) {
    const float4 x = s4[v];
    const float xs[4] = {x.x, x.y, x.z, x.w};
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int el = 4 * v + k;
      lds[(el / W) * WP + el % W] = xs[k];
    }
  }
  for (int el = 4 * nv + threadIdx.x; el < n; el += NT) lds[(el / W) * WP + el % W] = src[el];
}

template <int W, int WP>
GS_INLINE void stage_out(float *g, size_t row0, int rows, const float *lds) {
  float *dst = g + row0 * W;
  const int n = rows * W, nv = n >> 2;
  float4 *d4 = reinterpret_cast<float4 *>(dst);
  for (int v = threadIdx.x; v < nv; v += NT) {
    float xs[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int el = 4 * v + k;
      xs[k] = lds[(el / W) * WP + el % W];
    }
    d4[v] = make_float4(xs[0], xs[1], xs[2], xs[3]);
  }
  for (int el = 4 * nv + threadIdx.x; el < n; el += NT) dst[el] = lds[(el / W) * WP + el % W];
}

// Band L of a lane's row (coefficient k, channel c at my[3 k + c]) times M.
template <int L>
GS_INLINE void rotate_band(float *my, const float *M) {
  constexpr int n = 2 * L + 1;
  float m[n * n];
#pragma unroll
  for (int j = 0; j < n * n; ++j) m[j] = M[j];
#pragma unroll
  for (int c = 0; c < 3; ++c) {
    float in[n], out[n];
#pragma unroll
    for (int j = 0; j < n; ++j) in[j] = my[3 * j + c];
#pragma unroll
    for (int a = 0; a < n; ++a) {
      float acc = __fmul_rn(m[a * n], in[0]);
#pragma unroll
      for (int b = 1; b < n; ++b) acc = __fmaf_rn(m[a * n + b], in[b], acc);
      out[a] = acc;
    }
#pragma unroll
    for (int a = 0; a < n; ++a) my[3 * a + c] = out[a];
  }
}

template <int DEG, bool IDS, bool GEOM>
__global__ void __launch_bounds__(NT)
apply_kernel(int64_t N, int64_t S, const float *__restrict__ rec,
             const int32_t *__restrict__ status, const int64_t *__restrict__ ids,
             const float *means, const float *quats, const float *scales, const float *shN,
             float *o_means, float *o_quats, float *o_scales, float *o_shN,
             unsigned long long *counter) {
  constexpr int W = sh_words(DEG);
  constexpr int WP = W | 1;
  constexpr int RF = record_floats(DEG);
  __shared__ float sh[DEG ? NT * WP : 1];
  __shared__ float ms[GEOM ? NT * 3 : 1];
  __shared__ float ss[GEOM ? NT * 3 : 1];

  const size_t row0 = (size_t)blockIdx.x * NT;
  const int rows = (size_t)N - row0 < (size_t)NT ? (int)((size_t)N - row0) : NT;
  const int i = threadIdx.x;
  const size_t row = row0 + i;
  const bool live = i < rows;

  float4 q = make_float4(0.f, 0.f, 0.f, 0.f);
  if (GEOM && live) q = reinterpret_cast<const float4 *>(quats)[row];
  if constexpr (DEG > 0) stage_in<W, WP>(shN, row0, rows, sh);
  if (GEOM) {
    stage_in<3, 3>(means, row0, rows, ms);
    stage_in<3, 3>(scales, row0, rows, ss);
  }

  // the record is read only for a segment inside [0, S)
  int64_t seg = 0;
  bool ok = live, outside = false;
  if (IDS && live) {
    const int64_t id = ids[row];
    outside = id < 0 || id >= S;
    ok = !outside;
    seg = outside ? 0 : id;
  }
  if (ok) ok = status[seg] == 0;
  const float *r = rec + (size_t)seg * RF;
  if (IDS) {
    const unsigned long long m = __ballot(outside);
    if (m && (i & (kWave - 1)) == 0) atomicAdd(counter, (unsigned long long)__popcll(m));
  }
  __syncthreads();

  if (ok) {
    if (GEOM) {
      const float x = ms[3 * i], y = ms[3 * i + 1], z = ms[3 * i + 2];
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        ms[3 * i + k] = __fmaf_rn(r[3 * k], x, __fmaf_rn(r[3 * k + 1], y,
                                  __fmaf_rn(r[3 * k + 2], z, r[9 + k])));
        ss[3 * i + k] = __fadd_rn(ss[3 * i + k], r[16]);
      }
      const float aw = r[12], ax = r[13], ay = r[14], az = r[15];
      const float bw = q.x, bx = q.y, by = q.z, bz = q.w;
      q.x = __fmaf_rn(-az, bz, __fmaf_rn(-ay, by, __fmaf_rn(-ax, bx, __fmul_rn(aw, bw))));
      q.y = __fmaf_rn(-az, by, __fmaf_rn(ay, bz, __fmaf_rn(ax, bw, __fmul_rn(aw, bx))));
      q.z = __fmaf_rn(az, bx, __fmaf_rn(ay, bw, __fmaf_rn(-ax, bz, __fmul_rn(aw, by))));
      q.w = __fmaf_rn(az, bw, __fmaf_rn(-ay, bx, __fmaf_rn(ax, by, __fmul_rn(aw, bz))));
    }
    if (DEG) {
      float *my = sh + i * WP;
      if (DEG >= 1) rotate_band<1>(my, r + HDR);
      if (DEG >= 2) rotate_band<2>(my + 9, r + HDR + 9);
      if (DEG >= 3) rotate_band<3>(my + 24, r + HDR + 34);
      if (DEG >= 4) rotate_band<4>(my + 45, r + HDR + 83);
    }
  }
  if (GEOM && live) reinterpret_cast<float4 *>(o_quats)[row] = q;
  __syncthreads();

  if constexpr (DEG > 0) stage_out<W, WP>(o_shN, row0, rows, sh);
  if (GEOM) {
    stage_out<3, 3>(o_means, row0, rows, ms);
    stage_out<3, 3>(o_scales, row0, rows, ss);
  }
}

inline bool same_or_apart(const void *a, const void *b, uint64_t bytes) {
  const uintptr_t x = (uintptr_t)a, y = (uintptr_t)b;
  return x == y || x + bytes <= y || y + bytes <= x;
}

template <bool GEOM>
int launch_apply(int64_t N, int degree, int64_t S, const float *rec, const int32_t *status,
                 const int64_t *ids, const float *means, const float *quats, const float *scales,
                 const float *shN, float *o_means, float *o_quats, float *o_scales, float *o_shN,
                 unsigned long long *counter, hipStream_t st) {
  GS_HIP(zero_async(counter, 8, st));
  const dim3 grid((unsigned)((N + NT - 1) / NT)), block(NT);
#define GS_XF_CASE(D)                                                                            \
  case D:                                                                                        \
    if (ids)                                                                                     \
      hipLaunchKernelGGL((apply_kernel<D, true, GEOM>), grid, block, 0, st, N, S, rec, status,   \
                         ids, means, quats, scales, shN, o_means, o_quats, o_scales, o_shN,      \
                         counter);                                                               \
    else                                                                                         \
      hipLaunchKernelGGL((apply_kernel<D, false, GEOM>), grid, block, 0, st, N, S, rec, status,  \
                         ids, means, quats, scales, shN, o_means, o_quats, o_scales, o_shN,      \
                         counter);                                                               \
    break;
  switch (degree) {
    GS_XF_CASE(0)
    GS_XF_CASE(1)
    GS_XF_CASE(2)
    GS_XF_CASE(3)
    GS_XF_CASE(4)
  }
#undef GS_XF_CASE
  GS_CHECK_LAUNCH("splat_xform_apply");
  return 0;
}

}  // namespace xf
}  // namespace gs

using namespace gs;

extern "C" int gsplat_hip_splat_xform_record_floats(int degree) {
  return degree < 0 || degree > 4 ? 0 : xf::record_floats(degree);
}

extern "C" int gsplat_hip_splat_xform_prepare(int64_t S, int degree, const double *transforms,
                                              float *records, int32_t *status, void *stream) {
  GS_REQUIRE(S >= 1 && S < ((int64_t)1 << 31), "splat_xform_prepare: S %lld outside [1, 2^31)",
             (long long)S);
  GS_REQUIRE(degree >= 0 && degree <= 4, "splat_xform_prepare: degree %d outside [0, 4]", degree);
  GS_REQUIRE(transforms && records && status, "splat_xform_prepare: null pointer");
  hipStream_t st = (hipStream_t)stream;
  const dim3 grid((unsigned)((S + 63) / 64)), block(64);
  switch (degree) {
    case 0: hipLaunchKernelGGL(xf::prepare_kernel<0>, grid, block, 0, st, S, transforms, records, status); break;
    case 1: hipLaunchKernelGGL(xf::prepare_kernel<1>, grid, block, 0, st, S, transforms, records, status); break;
    case 2: hipLaunchKernelGGL(xf::prepare_kernel<2>, grid, block, 0, st, S, transforms, records, status); break;
    case 3: hipLaunchKernelGGL(xf::prepare_kernel<3>, grid, block, 0, st, S, transforms, records, status); break;
    default: hipLaunchKernelGGL(xf::prepare_kernel<4>, grid, block, 0, st, S, transforms, records, status); break;
  }
  GS_CHECK_LAUNCH("splat_xform_prepare");
  return 0;
}

static int xform_common_checks(const char *who, int64_t N, int degree, int64_t S,
                               const float *records, const int32_t *status, const float *shN,
                               float *out_shN, int64_t *counter) {
  GS_REQUIRE(N >= 1 && N < ((int64_t)1 << 37), "%s: N %lld outside [1, 2^37)", who, (long long)N);
  GS_REQUIRE(degree >= 0 && degree <= 4, "%s: degree %d outside [0, 4]", who, degree);
  GS_REQUIRE(S >= 1 && S < ((int64_t)1 << 31), "%s: S %lld outside [1, 2^31)", who, (long long)S);
  GS_REQUIRE(records && status && counter, "%s: null records, status or counter", who);
  GS_REQUIRE(((uintptr_t)counter & 7) == 0, "%s: counter must be 8-B aligned", who);
  if (degree > 0) {
    GS_REQUIRE(shN && out_shN, "%s: null shN or out_shN at degree %d", who, degree);
    GS_REQUIRE((((uintptr_t)shN | (uintptr_t)out_shN) & 15) == 0,
               "%s: shN and out_shN must be 16-B aligned", who);
    GS_REQUIRE(xf::same_or_apart(shN, out_shN, (uint64_t)N * xf::sh_words(degree) * 4),
               "%s: out_shN must be shN itself or not overlap it", who);
  }
  return 0;
}

extern "C" int gsplat_hip_splat_xform_apply(int64_t N, int degree, int64_t S, const float *records,
                                            const int32_t *status, const int64_t *segment_ids,
                                            const float *means, const float *quats,
                                            const float *scales, const float *shN,
                                            float *out_means, float *out_quats, float *out_scales,
                                            float *out_shN, int64_t *counter, void *stream) {
  const char *who = "splat_xform_apply";
  if (int rc = xform_common_checks(who, N, degree, S, records, status, shN, out_shN, counter))
    return rc;
  GS_REQUIRE(means && quats && scales && out_means && out_quats && out_scales,
             "%s: null means, quats, scales or one of their outputs", who);
  GS_REQUIRE((((uintptr_t)means | (uintptr_t)quats | (uintptr_t)scales | (uintptr_t)out_means |
               (uintptr_t)out_quats | (uintptr_t)out_scales) & 15) == 0,
             "%s: means, quats, scales and their outputs must be 16-B aligned", who);
  GS_REQUIRE(xf::same_or_apart(means, out_means, (uint64_t)N * 12) &&
                 xf::same_or_apart(quats, out_quats, (uint64_t)N * 16) &&
                 xf::same_or_apart(scales, out_scales, (uint64_t)N * 12),
             "%s: an output must be its input itself or not overlap it", who);
  return xf::launch_apply<true>(N, degree, S, records, status, segment_ids, means, quats, scales,
                                shN, out_means, out_quats, out_scales, out_shN,
                                reinterpret_cast<unsigned long long *>(counter),
                                (hipStream_t)stream);
}

extern "C" int gsplat_hip_splat_xform_rotate_sh(int64_t N, int degree, int64_t S,
                                                const float *records, const int32_t *status,
                                                const int64_t *segment_ids, const float *shN,
                                                float *out_shN, int64_t *counter, void *stream) {
  const char *who = "splat_xform_rotate_sh";
  if (int rc = xform_common_checks(who, N, degree, S, records, status, shN, out_shN, counter))
    return rc;
  GS_REQUIRE(degree >= 1, "%s: degree 0 has nothing to rotate", who);
  return xf::launch_apply<false>(N, degree, S, records, status, segment_ids, nullptr, nullptr,
                                 nullptr, shN, nullptr, nullptr, nullptr, out_shN,
                                 reinterpret_cast<unsigned long long *>(counter),
                                 (hipStream_t)stream);
}
