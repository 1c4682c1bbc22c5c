// Projection stage for Gaussians given by covariances, for gfx950:
//
//   * the fused EWA projection (pinhole) from covars [N,6] (upper triangle
//     xx, xy, xz, yy, yz, zz), dense and packed, forward and backward
//     (gsplat/cuda/csrc/ProjectionEWA3DGSFused.cu:74-98,453-464,
//     ProjectionEWA3DGSPacked.cu);
//   * the unfused stages world_to_cam and proj (pinhole / ortho / fisheye)
//     with their VJPs (gsplat/cuda/_wrapper.py:19-53,176-206,
//     gsplat/cuda/_torch_impl.py:71-247).
//
// All kernels are one lane per (camera, Gaussian) pair, streaming: no LDS
// beyond the view-matrix reductions.  The grid is (ceil(N/256), C) so the
// camera parameters are wave-uniform scalar loads.  The camera and the pinhole
// EWA algebra, forward and VJP, are proj_math.h's, shared with projection.hip;
// this file adds the [N,6] rows, the stages and the other camera models.
#include "common.h"
#include "proj_math.h"
#include "../../include/gsplat_hip.h"

namespace gs {
namespace cv {

// Symmetric 3x3 from a [N,6] row.  Rows are 24 B: 8-B aligned, three float2.
GS_INLINE M3 load_covar6(const float *__restrict__ covars, size_t n) {
  const float2 *p = reinterpret_cast<const float2 *>(covars + 6 * n);
  const float2 a = p[0], b = p[1], c = p[2];
  M3 m;
  m.m[0][0] = a.x;
  m.m[0][1] = m.m[1][0] = a.y;
  m.m[0][2] = m.m[2][0] = b.x;
  m.m[1][1] = b.y;
  m.m[1][2] = m.m[2][1] = c.x;
  m.m[2][2] = c.y;
  return m;
}

// ===================================================== fused, from covars ==
struct FwdArgs {
  int C, N, W, H;
  float eps2d, near_plane, far_plane, radius_clip;
  const float *means, *covars, *viewmats, *Ks;
  int32_t *radii;
  float *means2d, *depths, *conics, *comps;  // comps may be null
  // packed mode: per-block counts of kept pairs, then their exclusive prefix
  int64_t *block_cnt;
  const int64_t *block_off;
  int64_t *camera_ids, *gaussian_ids;
};

// MODE 0 / 1 / 2: dense outputs, packed count, packed write (ewa_fwd_tail).
template <int MODE>
__global__ void __launch_bounds__(256) covar_fwd_kernel(FwdArgs a) {
  const int c = blockIdx.y;
  const int n_raw = blockIdx.x * blockDim.x + threadIdx.x;
  const Cam k = load_cam(a.viewmats, a.Ks, c);
  if (MODE == 0 && n_raw >= a.N) return;
  const bool in = n_raw < a.N;
  const int n = in ? n_raw : a.N - 1;  // packed modes: every lane reaches the block scan
  const M3 C3 = load_covar6(a.covars, (size_t)n);
  const float *mp = a.means + 3 * (size_t)n;
  ewa_fwd<MODE>(a, k, c, n, in, mp[0], mp[1], mp[2], C3);
}

struct BwdArgs {
  int C, N, W, H;
  float eps2d;
  const float *means, *covars, *viewmats, *Ks;
  const int32_t *radii;
  const float *conics, *comps;                             // comps may be null
  const float *v_means2d, *v_depths, *v_conics, *v_comps;  // v_depths, v_comps may be null
  float *v_means, *v_covars, *v_viewmats;                  // v_viewmats may be null
  int store_mode;  // 1: C == 1, every lane stores its own row (no atomics, no zero fill)
  // packed: entry e is the pair (camera_ids[e], gaussian_ids[e]); sparse:
  // per-entry gradient rows [nnz, .]
  const int64_t *camera_ids, *gaussian_ids;
  int64_t nnz;
  int sparse;
};

GS_INLINE void store_covar6(float *__restrict__ v_covars, size_t row, const float (&vc)[6]) {
  float2 *o = reinterpret_cast<float2 *>(v_covars + 6 * row);
  o[0] = make_float2(vc[0], vc[1]);
  o[1] = make_float2(vc[2], vc[3]);
  o[2] = make_float2(vc[4], vc[5]);
}

__global__ void __launch_bounds__(256) covar_bwd_kernel(BwdArgs a) {
  const bool packed = a.camera_ids != nullptr;
  const PairIdx pr = decode_pair(a, packed, blockDim.x);
  const int c = pr.c, n = pr.n;
  const size_t idx = pr.idx;
  const bool valid = pr.valid;
  const Cam k = load_cam(a.viewmats, a.Ks, c);

  float vR[3][3] = {{0.f}}, vt[3] = {0.f, 0.f, 0.f};
  float vm[3] = {0.f, 0.f, 0.f}, vc6[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};

  if (valid) {
    const Sym2 d = conic_blur_vjp(a, idx);
    // ---- recompute the forward intermediates
    const M3 C3 = load_covar6(a.covars, (size_t)n);
    const float *mp = a.means + 3 * (size_t)n;
    const float m[3] = {mp[0], mp[1], mp[2]};
    float mc[3];
    world_to_cam_mean(k, m[0], m[1], m[2], mc);
    const M3 Cc = mul(mul(k.R, C3), transpose(k.R));
    const ProjOut p = persp(mc[0], mc[1], mc[2], Cc, k, a.W, a.H);

    M3 v3;
    float vmc[3];
    persp_vjp<false>(p, k, mc, Cc, d, a.v_means2d[2 * idx], a.v_means2d[2 * idx + 1], v3, vmc);
    if (a.v_depths) vmc[2] += a.v_depths[idx];  // null: depths unused downstream
    const M3 vC3 = world_to_cam_vjp(k, C3, m, v3, vmc, a.v_viewmats != nullptr, vm, vR, vt);
    // ---- upper triangle: diagonal as it is, off-diagonal v[i][j] + v[j][i]
    vc6[0] = vC3.m[0][0];
    vc6[1] = vC3.m[0][1] + vC3.m[1][0];
    vc6[2] = vC3.m[0][2] + vC3.m[2][0];
    vc6[3] = vC3.m[1][1];
    vc6[4] = vC3.m[1][2] + vC3.m[2][1];
    vc6[5] = vC3.m[2][2];
  }

  if (a.sparse) {
    if (valid) {  // COO values, one row per packed entry
      float *o = a.v_means + 3 * idx;
      o[0] = vm[0]; o[1] = vm[1]; o[2] = vm[2];
      store_covar6(a.v_covars, idx, vc6);
    }
  } else if (a.store_mode) {
    if (n < a.N) {
      float *o = a.v_means + 3 * (size_t)n;
      o[0] = vm[0]; o[1] = vm[1]; o[2] = vm[2];
      store_covar6(a.v_covars, (size_t)n, vc6);
    }
  } else if (valid) {
#pragma unroll
    for (int j = 0; j < 3; ++j) atomic_add_f32(a.v_means + 3 * (size_t)n + j, vm[j]);
#pragma unroll
    for (int j = 0; j < 6; ++j) atomic_add_f32(a.v_covars + 6 * (size_t)n + j, vc6[j]);
  }
  reduce_v_viewmats(a.v_viewmats, packed, valid, c, vR, vt);
}

// ========================================================== world_to_cam ==
// means_c = R m + t, covars_c = R S R^T for a general 3x3 S.
__global__ void __launch_bounds__(256) world_to_cam_fwd_kernel(
    int N, const float *__restrict__ means, const float *__restrict__ covars,
    const float *__restrict__ viewmats, float *__restrict__ means_c,
    float *__restrict__ covars_c) {
  const int c = blockIdx.y;
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  Cam k;
  load_view(k, viewmats, c);
  if (n >= N) return;
  const size_t idx = (size_t)c * N + n;
  if (means_c) {
    const float *mp = means + 3 * (size_t)n;
    const float m0 = mp[0], m1 = mp[1], m2 = mp[2];
    float *o = means_c + 3 * idx;
#pragma unroll
    for (int i = 0; i < 3; ++i)
      o[i] = k.R.m[i][0] * m0 + k.R.m[i][1] * m1 + k.R.m[i][2] * m2 + k.t[i];
  }
  if (covars_c) {
    M3 S;
    const float *sp = covars + 9 * (size_t)n;
#pragma unroll
    for (int i = 0; i < 9; ++i) S.m[i / 3][i % 3] = sp[i];
    const M3 Sc = mul(mul(k.R, S), transpose(k.R));
    float *o = covars_c + 9 * idx;
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] = Sc.m[i / 3][i % 3];
  }
}

// One lane per Gaussian walking the cameras: v_means and v_covars are summed
// in registers and stored once (no atomics, no zero fill, a fixed order); the
// 12 view-matrix partials of each camera are block-reduced, then one atomic
// per block and element into the zero-filled v_viewmats.
//   v_m = R^T v_mc;  v_S = R^T V R;  v_R = v_mc m^T + V R S^T + V^T R S;  v_t = v_mc
__global__ void __launch_bounds__(256) world_to_cam_bwd_kernel(
    int C, int N, const float *__restrict__ means, const float *__restrict__ covars,
    const float *__restrict__ viewmats, const float *__restrict__ v_means_c,
    const float *__restrict__ v_covars_c, float *__restrict__ v_means,
    float *__restrict__ v_covars, float *__restrict__ v_viewmats) {
  __shared__ float red[4][12];
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  const bool in = n < N;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  float m[3] = {0.f, 0.f, 0.f};
  M3 S;
#pragma unroll
  for (int i = 0; i < 9; ++i) S.m[i / 3][i % 3] = 0.f;
  if (in && v_viewmats) {
    const float *mp = means + 3 * (size_t)n;
    m[0] = mp[0]; m[1] = mp[1]; m[2] = mp[2];
    const float *sp = covars + 9 * (size_t)n;
#pragma unroll
    for (int i = 0; i < 9; ++i) S.m[i / 3][i % 3] = sp[i];
  }
  float vm[3] = {0.f, 0.f, 0.f};
  M3 vS;
#pragma unroll
  for (int i = 0; i < 9; ++i) vS.m[i / 3][i % 3] = 0.f;

  for (int c = 0; c < C; ++c) {
    Cam k;
    load_view(k, viewmats, c);
    const size_t idx = (size_t)c * N + (in ? n : 0);
    float vmc[3] = {0.f, 0.f, 0.f};
    M3 V;
#pragma unroll
    for (int i = 0; i < 9; ++i) V.m[i / 3][i % 3] = 0.f;
    if (in && v_means_c) {
      const float *p = v_means_c + 3 * idx;
      vmc[0] = p[0]; vmc[1] = p[1]; vmc[2] = p[2];
    }
    if (in && v_covars_c) {
      const float *p = v_covars_c + 9 * idx;
#pragma unroll
      for (int i = 0; i < 9; ++i) V.m[i / 3][i % 3] = p[i];
    }
    if (v_means) {
#pragma unroll
      for (int j = 0; j < 3; ++j)
        vm[j] += k.R.m[0][j] * vmc[0] + k.R.m[1][j] * vmc[1] + k.R.m[2][j] * vmc[2];
    }
    if (v_covars) {
      const M3 t = mul(mul(transpose(k.R), V), k.R);
#pragma unroll
      for (int i = 0; i < 9; ++i) vS.m[i / 3][i % 3] += t.m[i / 3][i % 3];
    }
    if (v_viewmats) {  // uniform: every lane of the block takes part
      const M3 a1 = mul(mul(V, k.R), transpose(S));
      const M3 a2 = mul(mul(transpose(V), k.R), S);
      float v[12];
#pragma unroll
      for (int i = 0; i < 3; ++i) {
#pragma unroll
        for (int j = 0; j < 3; ++j) v[i * 4 + j] = vmc[i] * m[j] + a1.m[i][j] + a2.m[i][j];
        v[i * 4 + 3] = vmc[i];
      }
#pragma unroll
      for (int e = 0; e < 12; ++e) v[e] = wave_sum(v[e]);
      if (lane == 0) {
#pragma unroll
        for (int e = 0; e < 12; ++e) red[wid][e] = v[e];
      }
      __syncthreads();
      if (threadIdx.x < 12) {
        const float s = ((red[0][threadIdx.x] + red[1][threadIdx.x]) + red[2][threadIdx.x]) +
                        red[3][threadIdx.x];
        if (s != 0.f) atomic_add_f32(v_viewmats + c * 16 + threadIdx.x, s);
      }
      __syncthreads();  // red is reused by the next camera
    }
  }
  if (!in) return;
  if (v_means) {
    float *o = v_means + 3 * (size_t)n;
    o[0] = vm[0]; o[1] = vm[1]; o[2] = vm[2];
  }
  if (v_covars) {
    float *o = v_covars + 9 * (size_t)n;
#pragma unroll
    for (int i = 0; i < 9; ++i) o[i] = vS.m[i / 3][i % 3];
  }
}

// ================================================================== proj ==
// means2d and the 2x3 Jacobian J of one camera model; covars2d = J S J^T.
enum { kPinhole = 0, kOrtho = 1, kFisheye = 2 };

struct Jac {
  float j[2][3];
  float mx, my;
};

// The scalars of the fisheye (equidistant) model and, for the VJP, their
// derivatives.  The model is the reference's, with its 1e-7 regularisers
// (e below): L = |xy| + e, U = |xy|^2 + e,
//   means2d = f * (x, y) * G1 + c,      G1 = atan2(L, z + e) / L
//   J = [ fx (x2 D + gB)   fx xy D          -fx x Q ]   gB = atan2(L, z) / L
//       [ fy xy D          fy (y2 D + gB)   -fy y Q ]   Q  = 1 / (U + z^2)
// with x2 = x^2 + e, y2 = y^2 and D = (z Q - gB) / U.  That is the reference's
// (a, b) form rewritten through D = a - b and U b = gB, which leaves D and the
// bracket B of its derivative as the only differences of nearly equal terms:
// near the optical axis z Q and gB agree to |xy|^2 / z^2.  This scalar chain
// (a dozen values per lane) runs in float64, where those differences keep
// ten digits down to |xy| / z = 1e-3; the matrix algebra stays fp32.
struct Fish {
  float G1, gB, D, Q;
  // VJP only
  float dD_xy;   // dD/dx = x * dD_xy, dD/dy = y * dD_xy
  float dD_z;
  float dgB_xy;  // dgB/dx = x * dgB_xy
  float QL;      // dgB/dz = -QL
  float dG1_xy;  // dG1/dx = x * dG1_xy
  float Q1;      // dG1/dz = -Q1
};

template <bool VJP>
GS_INLINE Fish fisheye_scalars(float xf, float yf, float zf) {
  const double e = 1e-7;
  const double x = xf, y = yf, z = zf;
  const double u0 = x * x + y * y;
  const double r0 = sqrt(u0);
  const double L = r0 + e, U = u0 + e, L2 = L * L;
  const double z1 = z + e;
  const double G1 = atan2(L, z1) / L;
  const double gB = atan2(L, z) / L;
  const double Q = 1.0 / (U + z * z);
  const double D = (z * Q - gB) / U;
  Fish f;
  f.G1 = (float)G1;
  f.gB = (float)gB;
  f.D = (float)D;
  f.Q = (float)Q;
  if (VJP) {
    const double QL = 1.0 / (L2 + z * z);
    const double HB = (z * QL - gB) / L2;      // (dgB/dL) / L
    const double Q1 = 1.0 / (L2 + z1 * z1);
    const double H1 = (z1 * Q1 - G1) / L2;     // (dG1/dL) / L
    const double Lrho = r0 > 0.0 ? L / r0 : 0.0;  // L * dL/dx / x; |xy| = 0: no direction
    const double B = 2.0 * z * Q * Q + HB * Lrho + 2.0 * D;
    f.dD_xy = (float)(-B / U);
    f.dD_z = (float)(2.0 * Q * Q + (U - L2) / U * Q * QL);
    f.dgB_xy = (float)(HB * Lrho);
    f.QL = (float)QL;
    f.dG1_xy = (float)(H1 * Lrho);
    f.Q1 = (float)Q1;
  }
  return f;
}

GS_INLINE Jac jac_pinhole(float x, float y, const PinClamp &p, const Cam &k) {
  Jac o;
  o.j[0][0] = k.fx * p.iz; o.j[0][1] = 0.f; o.j[0][2] = -k.fx * p.sx * p.iz;
  o.j[1][0] = 0.f; o.j[1][1] = k.fy * p.iz; o.j[1][2] = -k.fy * p.sy * p.iz;
  o.mx = k.fx * x * p.iz + k.cx;
  o.my = k.fy * y * p.iz + k.cy;
  return o;
}

GS_INLINE Jac jac_ortho(float x, float y, const Cam &k) {
  Jac o;
  o.j[0][0] = k.fx; o.j[0][1] = 0.f; o.j[0][2] = 0.f;
  o.j[1][0] = 0.f; o.j[1][1] = k.fy; o.j[1][2] = 0.f;
  o.mx = k.fx * x + k.cx;
  o.my = k.fy * y + k.cy;
  return o;
}

GS_INLINE Jac jac_fisheye(float x, float y, const Fish &f, const Cam &k) {
  const float e = 1e-7f;
  const float x2 = x * x + e, y2 = y * y, xy = x * y;
  Jac o;
  o.j[0][0] = k.fx * (x2 * f.D + f.gB);
  o.j[0][1] = k.fx * xy * f.D;
  o.j[0][2] = -k.fx * x * f.Q;
  o.j[1][0] = k.fy * xy * f.D;
  o.j[1][1] = k.fy * (y2 * f.D + f.gB);
  o.j[1][2] = -k.fy * y * f.Q;
  o.mx = k.fx * x * f.G1 + k.cx;
  o.my = k.fy * y * f.G1 + k.cy;
  return o;
}

template <int MODEL>
__global__ void __launch_bounds__(256) proj_fwd_kernel(
    int N, int W, int H, const float *__restrict__ means, const float *__restrict__ covars,
    const float *__restrict__ Ks, float *__restrict__ means2d, float *__restrict__ covars2d) {
  const int c = blockIdx.y;
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  Cam k;
  load_K(k, Ks, c);
  if (n >= N) return;
  const size_t idx = (size_t)c * N + n;
  const float *mp = means + 3 * idx;
  const float x = mp[0], y = mp[1], z = mp[2];
  const float *sp = covars + 9 * idx;
  float S[3][3];
#pragma unroll
  for (int i = 0; i < 9; ++i) S[i / 3][i % 3] = sp[i];
  Jac J;
  if (MODEL == kPinhole) J = jac_pinhole(x, y, pin_clamp(x, y, z, k, W, H), k);
  else if (MODEL == kOrtho) J = jac_ortho(x, y, k);
  else J = jac_fisheye(x, y, fisheye_scalars<false>(x, y, z), k);
  float JS[2][3];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int b = 0; b < 3; ++b)
      JS[i][b] = J.j[i][0] * S[0][b] + J.j[i][1] * S[1][b] + J.j[i][2] * S[2][b];
  float c2[4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int l = 0; l < 2; ++l)
      c2[i * 2 + l] = JS[i][0] * J.j[l][0] + JS[i][1] * J.j[l][1] + JS[i][2] * J.j[l][2];
  *reinterpret_cast<float2 *>(means2d + 2 * idx) = make_float2(J.mx, J.my);
  *reinterpret_cast<float4 *>(covars2d + 4 * idx) = make_float4(c2[0], c2[1], c2[2], c2[3]);
}

// v_S = J^T G J and v_J = G J S^T + G^T J S for a general 2x2 cotangent G and
// a general 3x3 S; then the model's chain from (v_means2d, v_J) to v_means.
template <int MODEL>
__global__ void __launch_bounds__(256) proj_bwd_kernel(
    int N, int W, int H, const float *__restrict__ means, const float *__restrict__ covars,
    const float *__restrict__ Ks, const float *__restrict__ v_means2d,
    const float *__restrict__ v_covars2d, float *__restrict__ v_means,
    float *__restrict__ v_covars) {
  const int c = blockIdx.y;
  const int n = blockIdx.x * blockDim.x + threadIdx.x;
  Cam k;
  load_K(k, Ks, c);
  if (n >= N) return;
  const size_t idx = (size_t)c * N + n;
  const float *mp = means + 3 * idx;
  const float x = mp[0], y = mp[1], z = mp[2];
  float a = 0.f, b = 0.f, G[2][2] = {{0.f, 0.f}, {0.f, 0.f}};
  if (v_means2d) {
    const float2 t = *reinterpret_cast<const float2 *>(v_means2d + 2 * idx);
    a = t.x;
    b = t.y;
  }
  if (v_covars2d) {
    const float4 t = *reinterpret_cast<const float4 *>(v_covars2d + 4 * idx);
    G[0][0] = t.x; G[0][1] = t.y; G[1][0] = t.z; G[1][1] = t.w;
  }
  PinClamp pc;
  Fish f;
  Jac J;
  if (MODEL == kPinhole) {
    pc = pin_clamp(x, y, z, k, W, H);
    J = jac_pinhole(x, y, pc, k);
  } else if (MODEL == kOrtho) {
    J = jac_ortho(x, y, k);
  } else {
    f = fisheye_scalars<true>(x, y, z);
    J = jac_fisheye(x, y, f, k);
  }
  float GJ[2][3], GtJ[2][3];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      GJ[i][q] = G[i][0] * J.j[0][q] + G[i][1] * J.j[1][q];
      GtJ[i][q] = G[0][i] * J.j[0][q] + G[1][i] * J.j[1][q];
    }
  if (v_covars) {
    float *o = v_covars + 9 * idx;
#pragma unroll
    for (int p = 0; p < 3; ++p)
#pragma unroll
      for (int q = 0; q < 3; ++q) o[p * 3 + q] = J.j[0][p] * GJ[0][q] + J.j[1][p] * GJ[1][q];
  }
  if (!v_means) return;
  float vx, vy, vz;
  if (MODEL == kOrtho) {  // J is constant
    vx = k.fx * a;
    vy = k.fy * b;
    vz = 0.f;
  } else {
    const float *sp = covars + 9 * idx;
    float S[3][3];
#pragma unroll
    for (int i = 0; i < 9; ++i) S[i / 3][i % 3] = sp[i];
    float vJ[2][3];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 3; ++q)
        vJ[i][q] = GJ[i][0] * S[q][0] + GJ[i][1] * S[q][1] + GJ[i][2] * S[q][2] +
                   GtJ[i][0] * S[0][q] + GtJ[i][1] * S[1][q] + GtJ[i][2] * S[2][q];
    if (MODEL == kPinhole) {
      // J00 = fx / z, J02 = -fx sx / z (sx = x / z, constant once clamped)
      const float iz = pc.iz, iz2 = iz * iz;
      vx = k.fx * iz * a + (pc.cx ? 0.f : -k.fx * iz2 * vJ[0][2]);
      vy = k.fy * iz * b + (pc.cy ? 0.f : -k.fy * iz2 * vJ[1][2]);
      vz = -(k.fx * x * a + k.fy * y * b) * iz2 - (k.fx * vJ[0][0] + k.fy * vJ[1][1]) * iz2 +
           (pc.cx ? 1.f : 2.f) * k.fx * pc.sx * iz2 * vJ[0][2] +
           (pc.cy ? 1.f : 2.f) * k.fy * pc.sy * iz2 * vJ[1][2];
    } else {
      const float e = 1e-7f;
      const float x2 = x * x + e, y2 = y * y, xy = x * y;
      const float fx = k.fx, fy = k.fy;
      const float vD = fx * (x2 * vJ[0][0] + xy * vJ[0][1]) + fy * (xy * vJ[1][0] + y2 * vJ[1][1]);
      const float vg = fx * vJ[0][0] + fy * vJ[1][1];
      const float vQ = -(fx * x * vJ[0][2] + fy * y * vJ[1][2]);
      // through the scalars D, gB, Q
      const float sxy = vD * f.dD_xy + vg * f.dgB_xy - 2.f * f.Q * f.Q * vQ;
      vx = x * sxy;
      vy = y * sxy;
      vz = vD * f.dD_z - vg * f.QL - 2.f * z * f.Q * f.Q * vQ;
      // the explicit x, y of J
      vx += fx * (2.f * x * f.D * vJ[0][0] + y * f.D * vJ[0][1] - f.Q * vJ[0][2]) +
            fy * (y * f.D * vJ[1][0]);
      vy += fx * (x * f.D * vJ[0][1]) +
            fy * (x * f.D * vJ[1][0] + 2.f * y * f.D * vJ[1][1] - f.Q * vJ[1][2]);
      // means2d
      const float w = a * fx * x + b * fy * y;
      vx += a * fx * f.G1 + x * f.dG1_xy * w;
      vy += b * fy * f.G1 + y * f.dG1_xy * w;
      vz -= w * f.Q1;
    }
  }
  float *o = v_means + 3 * idx;
  o[0] = vx; o[1] = vy; o[2] = vz;
}

}  // namespace cv
}  // namespace gs

using namespace gs;
using namespace gs::cv;

#define COVAR_ALIGNED(p) (((uintptr_t)(p) & 7) == 0)

extern "C" int gsplat_hip_projection_covar_fwd(
    int C, int N, const float *means, const float *covars, const float *viewmats,
    const float *Ks, int width, int height, float eps2d, float near_plane, float far_plane,
    float radius_clip, int32_t *radii, float *means2d, float *depths, float *conics,
    float *compensations, void *stream) {
  GS_REQUIRE(C >= 0 && N >= 0, "projection_covar_fwd: negative sizes C=%d N=%d", C, N);
  if (C == 0 || N == 0) return 0;
  GS_REQUIRE(C <= 65535, "projection_covar_fwd: C=%d exceeds the grid's 65535 cameras", C);
  GS_REQUIRE(means && covars && viewmats && Ks && radii && means2d && depths && conics,
             "projection_covar_fwd: null pointer argument");
  GS_REQUIRE(COVAR_ALIGNED(covars) && COVAR_ALIGNED(means2d),
             "projection_covar_fwd: covars and means2d must be 8-B aligned");
  FwdArgs a{C, N, width, height, eps2d, near_plane, far_plane, radius_clip,
            means, covars, viewmats, Ks, radii, means2d, depths, conics, compensations};
  dim3 grid((N + 255) / 256, C);
  hipLaunchKernelGGL(covar_fwd_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, a);
  GS_CHECK_LAUNCH("projection_covar_fwd");
  return 0;
}

extern "C" int gsplat_hip_projection_covar_bwd(
    int C, int N, const float *means, const float *covars, const float *viewmats,
    const float *Ks, int width, int height, float eps2d, const int32_t *radii,
    const float *conics, const float *compensations, const float *v_means2d,
    const float *v_depths, const float *v_conics, const float *v_compensations, float *v_means,
    float *v_covars, float *v_viewmats, void *stream) {
  GS_REQUIRE(C >= 0 && N >= 0, "projection_covar_bwd: negative sizes C=%d N=%d", C, N);
  GS_REQUIRE(C <= 65535, "projection_covar_bwd: C=%d exceeds the grid's 65535 cameras", C);
  hipStream_t st = (hipStream_t)stream;
  if (v_viewmats && C > 0) GS_HIP(gs::zero_async(v_viewmats, sizeof(float) * 16 * C, st));
  if (N == 0) return 0;
  GS_REQUIRE(v_means && v_covars, "projection_covar_bwd: null gradient output");
  const int store_mode = (C == 1);
  if (!store_mode) {
    GS_HIP(gs::zero_async(v_means, sizeof(float) * 3 * N, st));
    GS_HIP(gs::zero_async(v_covars, sizeof(float) * 6 * N, st));
  }
  if (C == 0) return 0;
  GS_REQUIRE(means && covars && viewmats && Ks && radii && conics && v_means2d && v_conics,
             "projection_covar_bwd: null pointer argument");
  GS_REQUIRE(!compensations == !v_compensations,
             "projection_covar_bwd: compensations and v_compensations must both be given or "
             "both null");
  GS_REQUIRE(COVAR_ALIGNED(covars) && COVAR_ALIGNED(v_covars),
             "projection_covar_bwd: covars / v_covars must be 8-B aligned");
  BwdArgs a{C, N, width, height, eps2d, means, covars, viewmats, Ks, radii, conics,
            compensations, v_means2d, v_depths, v_conics, v_compensations, v_means, v_covars,
            v_viewmats, store_mode, nullptr, nullptr, 0, 0};
  dim3 grid((N + 255) / 256, C);
  hipLaunchKernelGGL(covar_bwd_kernel, grid, dim3(256), 0, st, a);
  GS_CHECK_LAUNCH("projection_covar_bwd");
  return 0;
}

extern "C" int gsplat_hip_projection_covar_packed_count(
    int C, int N, const float *means, const float *covars, const float *viewmats,
    const float *Ks, int width, int height, float eps2d, float near_plane, float far_plane,
    float radius_clip, void *workspace, int64_t *nnz_device, void *stream) {
  GS_REQUIRE(C >= 0 && N >= 0, "projection_covar_packed_count: negative sizes C=%d N=%d", C, N);
  GS_REQUIRE(C <= 65535, "projection_covar_packed_count: C=%d exceeds 65535 cameras", C);
  GS_REQUIRE(nnz_device, "projection_covar_packed_count: null nnz_device");
  hipStream_t st = (hipStream_t)stream;
  if (C == 0 || N == 0) {
    GS_HIP(gs::zero_async(nnz_device, sizeof(int64_t), st));
    return 0;
  }
  GS_REQUIRE(means && covars && viewmats && Ks && workspace,
             "projection_covar_packed_count: null pointer argument");
  GS_REQUIRE(COVAR_ALIGNED(covars), "projection_covar_packed_count: covars must be 8-B aligned");
  FwdArgs a{C, N, width, height, eps2d, near_plane, far_plane, radius_clip,
            means, covars, viewmats, Ks, nullptr, nullptr, nullptr, nullptr, nullptr};
  a.block_cnt = reinterpret_cast<int64_t *>(workspace);
  dim3 grid((N + 255) / 256, C);
  hipLaunchKernelGGL(covar_fwd_kernel<1>, grid, dim3(256), 0, st, a);
  gs::launch_packed_scan((int64_t)grid.x * grid.y, a.block_cnt, nnz_device, st);
  GS_CHECK_LAUNCH("projection_covar_packed_count");
  return 0;
}

extern "C" int gsplat_hip_projection_covar_packed_fwd(
    int C, int N, const float *means, const float *covars, const float *viewmats,
    const float *Ks, int width, int height, float eps2d, float near_plane, float far_plane,
    float radius_clip, const void *workspace, int64_t *camera_ids, int64_t *gaussian_ids,
    int32_t *radii, float *means2d, float *depths, float *conics, float *compensations,
    void *stream) {
  GS_REQUIRE(C >= 0 && N >= 0, "projection_covar_packed_fwd: negative sizes C=%d N=%d", C, N);
  if (C == 0 || N == 0) return 0;
  GS_REQUIRE(C <= 65535, "projection_covar_packed_fwd: C=%d exceeds 65535 cameras", C);
  GS_REQUIRE(means && covars && viewmats && Ks && workspace && camera_ids && gaussian_ids &&
                 radii && means2d && depths && conics,
             "projection_covar_packed_fwd: null pointer argument");
  GS_REQUIRE(COVAR_ALIGNED(covars) && COVAR_ALIGNED(means2d),
             "projection_covar_packed_fwd: covars and means2d must be 8-B aligned");
  FwdArgs a{C, N, width, height, eps2d, near_plane, far_plane, radius_clip,
            means, covars, viewmats, Ks, radii, means2d, depths, conics, compensations};
  a.block_off = reinterpret_cast<const int64_t *>(workspace);
  a.camera_ids = camera_ids;
  a.gaussian_ids = gaussian_ids;
  dim3 grid((N + 255) / 256, C);
  hipLaunchKernelGGL(covar_fwd_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, a);
  GS_CHECK_LAUNCH("projection_covar_packed_fwd");
  return 0;
}

extern "C" int gsplat_hip_projection_covar_packed_bwd(
    int C, int N, int64_t nnz, const float *means, const float *covars, const float *viewmats,
    const float *Ks, int width, int height, float eps2d, const int64_t *camera_ids,
    const int64_t *gaussian_ids, const float *conics, const float *compensations,
    const float *v_means2d, const float *v_depths, const float *v_conics,
    const float *v_compensations, int sparse_grad, float *v_means, float *v_covars,
    float *v_viewmats, void *stream) {
  GS_REQUIRE(C >= 0 && N >= 0 && nnz >= 0, "projection_covar_packed_bwd: negative sizes");
  hipStream_t st = (hipStream_t)stream;
  if (v_viewmats && C > 0) GS_HIP(gs::zero_async(v_viewmats, sizeof(float) * 16 * C, st));
  if (!sparse_grad && N > 0) {
    GS_REQUIRE(v_means && v_covars, "projection_covar_packed_bwd: null gradient output");
    GS_HIP(gs::zero_async(v_means, sizeof(float) * 3 * N, st));
    GS_HIP(gs::zero_async(v_covars, sizeof(float) * 6 * N, st));
  }
  if (nnz == 0) return 0;
  GS_REQUIRE(nnz <= (int64_t)C * N, "projection_covar_packed_bwd: nnz exceeds C * N");
  GS_REQUIRE(!compensations == !v_compensations,
             "projection_covar_packed_bwd: compensations and v_compensations must both be "
             "given or both null");
  GS_REQUIRE(means && covars && viewmats && Ks && camera_ids && gaussian_ids && conics &&
                 v_means2d && v_conics && v_means && v_covars,
             "projection_covar_packed_bwd: null pointer argument");
  GS_REQUIRE(COVAR_ALIGNED(covars) && COVAR_ALIGNED(v_covars),
             "projection_covar_packed_bwd: covars / v_covars must be 8-B aligned");
  BwdArgs a{C, N, width, height, eps2d, means, covars, viewmats, Ks, nullptr, conics,
            compensations, v_means2d, v_depths, v_conics, v_compensations, v_means, v_covars,
            v_viewmats, 0, camera_ids, gaussian_ids, nnz, sparse_grad};
  hipLaunchKernelGGL(covar_bwd_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, a);
  GS_CHECK_LAUNCH("projection_covar_packed_bwd");
  return 0;
}

extern "C" int gsplat_hip_world_to_cam_fwd(int C, int N, const float *means, const float *covars,
                                           const float *viewmats, float *means_c,
                                           float *covars_c, void *stream) {
  GS_REQUIRE(C >= 0 && N >= 0, "world_to_cam_fwd: negative sizes C=%d N=%d", C, N);
  if (C == 0 || N == 0) return 0;
  GS_REQUIRE(C <= 65535, "world_to_cam_fwd: C=%d exceeds the grid's 65535 cameras", C);
  GS_REQUIRE(viewmats && (!means_c || means) && (!covars_c || covars),
             "world_to_cam_fwd: null pointer argument");
  dim3 grid((N + 255) / 256, C);
  hipLaunchKernelGGL(world_to_cam_fwd_kernel, grid, dim3(256), 0, (hipStream_t)stream, N, means,
                     covars, viewmats, means_c, covars_c);
  GS_CHECK_LAUNCH("world_to_cam_fwd");
  return 0;
}

extern "C" int gsplat_hip_world_to_cam_bwd(int C, int N, const float *means, const float *covars,
                                           const float *viewmats, const float *v_means_c,
                                           const float *v_covars_c, float *v_means,
                                           float *v_covars, float *v_viewmats, void *stream) {
  GS_REQUIRE(C >= 0 && N >= 0, "world_to_cam_bwd: negative sizes C=%d N=%d", C, N);
  hipStream_t st = (hipStream_t)stream;
  if (v_viewmats && C > 0) GS_HIP(gs::zero_async(v_viewmats, sizeof(float) * 16 * C, st));
  if (N == 0) return 0;
  GS_REQUIRE(viewmats || C == 0, "world_to_cam_bwd: null viewmats");
  GS_REQUIRE(!v_viewmats || (means && covars), "world_to_cam_bwd: v_viewmats needs means, covars");
  // C == 0: the kernel's camera loop is empty and it stores zeros
  hipLaunchKernelGGL(world_to_cam_bwd_kernel, dim3((N + 255) / 256), dim3(256), 0, st, C, N,
                     means, covars, viewmats, v_means_c, v_covars_c, v_means, v_covars,
                     v_viewmats);
  GS_CHECK_LAUNCH("world_to_cam_bwd");
  return 0;
}

extern "C" int gsplat_hip_proj_fwd(int C, int N, int camera_model, const float *means,
                                   const float *covars, const float *Ks, int width, int height,
                                   float *means2d, float *covars2d, void *stream) {
  GS_REQUIRE(C >= 0 && N >= 0, "proj_fwd: negative sizes C=%d N=%d", C, N);
  GS_REQUIRE(camera_model >= kPinhole && camera_model <= kFisheye,
             "proj_fwd: camera_model %d (0 pinhole, 1 ortho, 2 fisheye)", camera_model);
  if (C == 0 || N == 0) return 0;
  GS_REQUIRE(C <= 65535, "proj_fwd: C=%d exceeds the grid's 65535 cameras", C);
  GS_REQUIRE(means && covars && Ks && means2d && covars2d, "proj_fwd: null pointer argument");
  GS_REQUIRE(COVAR_ALIGNED(means2d) && ((uintptr_t)covars2d & 15) == 0,
             "proj_fwd: means2d must be 8-B aligned, covars2d 16-B aligned");
  dim3 grid((N + 255) / 256, C);
  hipStream_t st = (hipStream_t)stream;
  if (camera_model == kPinhole)
    hipLaunchKernelGGL(proj_fwd_kernel<kPinhole>, grid, dim3(256), 0, st, N, width, height, means,
                       covars, Ks, means2d, covars2d);
  else if (camera_model == kOrtho)
    hipLaunchKernelGGL(proj_fwd_kernel<kOrtho>, grid, dim3(256), 0, st, N, width, height, means,
                       covars, Ks, means2d, covars2d);
  else
    hipLaunchKernelGGL(proj_fwd_kernel<kFisheye>, grid, dim3(256), 0, st, N, width, height, means,
                       covars, Ks, means2d, covars2d);
  GS_CHECK_LAUNCH("proj_fwd");
  return 0;
}

extern "C" int gsplat_hip_proj_bwd(int C, int N, int camera_model, const float *means,
                                   const float *covars, const float *Ks, int width, int height,
                                   const float *v_means2d, const float *v_covars2d,
                                   float *v_means, float *v_covars, void *stream) {
  GS_REQUIRE(C >= 0 && N >= 0, "proj_bwd: negative sizes C=%d N=%d", C, N);
  GS_REQUIRE(camera_model >= kPinhole && camera_model <= kFisheye,
             "proj_bwd: camera_model %d (0 pinhole, 1 ortho, 2 fisheye)", camera_model);
  if (C == 0 || N == 0 || (!v_means && !v_covars)) return 0;
  GS_REQUIRE(C <= 65535, "proj_bwd: C=%d exceeds the grid's 65535 cameras", C);
  GS_REQUIRE(means && covars && Ks, "proj_bwd: null pointer argument");
  GS_REQUIRE(COVAR_ALIGNED(v_means2d) && ((uintptr_t)v_covars2d & 15) == 0,
             "proj_bwd: v_means2d must be 8-B aligned, v_covars2d 16-B aligned");
  dim3 grid((N + 255) / 256, C);
  hipStream_t st = (hipStream_t)stream;
  if (camera_model == kPinhole)
    hipLaunchKernelGGL(proj_bwd_kernel<kPinhole>, grid, dim3(256), 0, st, N, width, height, means,
                       covars, Ks, v_means2d, v_covars2d, v_means, v_covars);
  else if (camera_model == kOrtho)
    hipLaunchKernelGGL(proj_bwd_kernel<kOrtho>, grid, dim3(256), 0, st, N, width, height, means,
                       covars, Ks, v_means2d, v_covars2d, v_means, v_covars);
  else
    hipLaunchKernelGGL(proj_bwd_kernel<kFisheye>, grid, dim3(256), 0, st, N, width, height, means,
                       covars, Ks, v_means2d, v_covars2d, v_means, v_covars);
  GS_CHECK_LAUNCH("proj_bwd");
  return 0;
}
