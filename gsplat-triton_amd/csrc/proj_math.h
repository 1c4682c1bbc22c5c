// Camera and EWA-projection algebra shared by the projection kernels
// (projection.hip: Gaussians from quats / scales; projection_covar.hip: from
// covariances, and the unfused world_to_cam / proj stages).  Each piece of the
// pinhole projection and of its VJP is written once, here.
//
// projection.hip's kernels are pinned bit for bit by the training tests: a
// piece is used there only where the kernel compiles to the instructions it
// had with the text inline (tools/kernel_isa_diff.py, profiles/proj_math/).
#pragma once

#include "common.h"

namespace gs {

// the packed-count scan (projection.hip), also used by projection_covar.hip
// and the 2DGS packed projection (surfel_projection.hip)
void launch_packed_scan(int64_t nb, int64_t *cnt, int64_t *total, hipStream_t st);

struct Cam {
  M3 R;
  float t[3];
  float fx, fy, cx, cy;
};

GS_INLINE void load_view(Cam &k, const float *__restrict__ viewmats, int c) {
  const float *V = viewmats + c * 16;
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j) k.R.m[i][j] = V[i * 4 + j];
    k.t[i] = V[i * 4 + 3];
  }
}

GS_INLINE void load_K(Cam &k, const float *__restrict__ Ks, int c) {
  const float *K = Ks + c * 9;
  k.fx = K[0];
  k.fy = K[4];
  k.cx = K[2];
  k.cy = K[5];
}

GS_INLINE Cam load_cam(const float *__restrict__ viewmats, const float *__restrict__ Ks, int c) {
  Cam k;
  load_view(k, viewmats, c);
  load_K(k, Ks, c);
  return k;
}

// ---------------------------------------------------------- world -> camera
// (transform.py:38-119, 184-297)
GS_INLINE void world_to_cam_mean(const Cam &k, float m0, float m1, float m2, float (&mc)[3]) {
#pragma unroll
  for (int i = 0; i < 3; ++i)
    mc[i] = k.R.m[i][0] * m0 + k.R.m[i][1] * m1 + k.R.m[i][2] * m2 + k.t[i];
}

// VJP of mc = R m + t, Cc = R C3 R^T: vm = R^T vmc, the returned
// v_C3 = R^T v3 R and, where the view matrix takes a gradient, the partials
// vR = vmc m^T + 2 v3 R C3 (C3 symmetric) and vt = vmc.
GS_INLINE M3 world_to_cam_vjp(const Cam &k, const M3 &C3, const float (&m)[3], const M3 &v3,
                              const float (&vmc)[3], bool want_view, float (&vm)[3],
                              float (&vR)[3][3], float (&vt)[3]) {
#pragma unroll
  for (int j = 0; j < 3; ++j)
    vm[j] = k.R.m[0][j] * vmc[0] + k.R.m[1][j] * vmc[1] + k.R.m[2][j] * vmc[2];
  const M3 vSR = mul(v3, k.R);
  const M3 vC3 = mul(transpose(k.R), vSR);
  if (want_view) {
    const M3 vRc = mul(vSR, C3);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      vt[i] = vmc[i];
#pragma unroll
      for (int j = 0; j < 3; ++j) vR[i][j] = vmc[i] * m[j] + 2.f * vRc.m[i][j];
    }
  }
  return vC3;
}

// ------------------------------------------------------ pinhole projection
// x / z and y / z clamped to the image plus a 15 % margin; cx / cy: clamped.
struct PinClamp {
  float iz, sx, sy;
  bool cx, cy;
};

GS_INLINE PinClamp pin_clamp(float x, float y, float z, const Cam &k, int W, int H) {
  PinClamp p;
  p.iz = 1.f / z;
  float marx = 0.15f * (float)W / k.fx;
  float mary = 0.15f * (float)H / k.fy;
  float lox = -marx - k.cx / k.fx, hix = marx + ((float)W - k.cx) / k.fx;
  float loy = -mary - k.cy / k.fy, hiy = mary + ((float)H - k.cy) / k.fy;
  float sx = x * p.iz, sy = y * p.iz;
  p.cx = (sx < lox) | (sx > hix);
  p.cy = (sy < loy) | (sy > hiy);
  p.sx = fminf(fmaxf(sx, lox), hix);
  p.sy = fminf(fmaxf(sy, loy), hiy);
  return p;
}

struct ProjOut {
  float mx, my;             // projected mean
  float cxx, cxy, cyy;      // 2D covariance (before blur)
  float Jxx, Jxz, Jyy, Jyz; // Jacobian (clamped screen coordinates)
  bool clamp_x, clamp_y;
};

// Pinhole projection of a symmetric camera-space covariance with the
// screen-margin clamp (cam_proj.py:5-81).
GS_INLINE ProjOut persp(float x, float y, float z, const M3 &Cc, const Cam &k, int W, int H) {
  ProjOut o;
  const PinClamp s = pin_clamp(x, y, z, k, W, H);
  const float iz = s.iz;
  o.clamp_x = s.cx;
  o.clamp_y = s.cy;
  o.Jxx = k.fx * iz;
  o.Jxz = -k.fx * s.sx * iz;
  o.Jyy = k.fy * iz;
  o.Jyz = -k.fy * s.sy * iz;
  const float(*c)[3] = Cc.m;
  o.cxx = o.Jxx * c[0][0] * o.Jxx + 2.f * o.Jxx * c[0][2] * o.Jxz + o.Jxz * c[2][2] * o.Jxz;
  o.cxy = o.Jxx * (c[0][1] * o.Jyy + c[0][2] * o.Jyz) + o.Jxz * (c[1][2] * o.Jyy + c[2][2] * o.Jyz);
  o.cyy = o.Jyy * c[1][1] * o.Jyy + 2.f * o.Jyy * c[1][2] * o.Jyz + o.Jyz * c[2][2] * o.Jyz;
  o.mx = k.fx * x * iz + k.cx;
  o.my = k.fy * y * iz + k.cy;
  return o;
}

// ------------------------------------------------------------ forward tail
// From the projected pair to its outputs: blur (util_kernels.py:64-94),
// determinant, radius, culling, then the stores.  `keep` arrives holding the
// depth test.  MODE 0: dense [C, N] outputs at idx.  MODE 1: count the kept
// pairs per block.  MODE 2: write the kept pairs packed at
// block_off[block] + rank in block (wave ballots).  Args: ProjFwdArgs or
// cv::FwdArgs.
template <int MODE, class Args>
GS_INLINE void ewa_fwd_tail(const Args &a, int c, int n, size_t idx, bool keep, float depth,
                            const ProjOut &p) {
  const float det0 = p.cxx * p.cyy - p.cxy * p.cxy;
  const float bxx = p.cxx + a.eps2d, byy = p.cyy + a.eps2d;
  const float det = bxx * byy - p.cxy * p.cxy;
  keep &= det > 0.f;
  const float inv_det = 1.f / det;
  const float b = 0.5f * (bxx + byy);
  const float v1 = b + sqrtf(fmaxf(0.01f, b * b - det));
  const float r = ceilf(3.f * sqrtf(v1));
  keep &= (r > a.radius_clip) & (p.mx + r > 0.f) & (p.mx - r < (float)a.W) &
          (p.my + r > 0.f) & (p.my - r < (float)a.H);

  if (MODE == 0) {
    a.radii[idx] = keep ? (int32_t)r : 0;
    float2 m2d = keep ? make_float2(p.mx, p.my) : make_float2(0.f, 0.f);
    *reinterpret_cast<float2 *>(a.means2d + 2 * idx) = m2d;
    float *cn = a.conics + 3 * idx;
    cn[0] = keep ? inv_det * byy : 0.f;
    cn[1] = keep ? -inv_det * p.cxy : 0.f;
    cn[2] = keep ? inv_det * bxx : 0.f;
    if (a.comps) a.comps[idx] = keep ? sqrtf(fmaxf(det0 / det, 0.f)) : 0.f;
    return;
  }
  // packed: rank of this pair among the block's kept pairs (wave ballots)
  __shared__ int wave_cnt[4];
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t m = __ballot(keep);
  if (lane == 0) wave_cnt[wid] = __popcll(m);
  __syncthreads();
  const int64_t blk = (int64_t)c * gridDim.x + blockIdx.x;
  if (MODE == 1) {
    if (threadIdx.x == 0) a.block_cnt[blk] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
    return;
  }
  if (!keep) return;
  int before = 0;
  for (int w = 0; w < wid; ++w) before += wave_cnt[w];
  const int64_t o = a.block_off[blk] + before +
                    __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                              __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0));
  a.camera_ids[o] = c;
  a.gaussian_ids[o] = n;
  a.radii[o] = (int32_t)r;
  *reinterpret_cast<float2 *>(a.means2d + 2 * o) = make_float2(p.mx, p.my);
  a.depths[o] = depth;
  float *cn = a.conics + 3 * o;
  cn[0] = inv_det * byy;
  cn[1] = -inv_det * p.cxy;
  cn[2] = inv_det * bxx;
  if (a.comps) a.comps[o] = sqrtf(fmaxf(det0 / det, 0.f));
}

// The forward from a world-space mean and symmetric covariance on: world ->
// camera, the depth test, persp, the tail.  `in`: the lane holds a Gaussian
// (the packed modes keep every lane for the block scan).
template <int MODE, class Args>
GS_INLINE void ewa_fwd(const Args &a, const Cam &k, int c, int n, bool in, float m0, float m1,
                       float m2, const M3 &C3) {
  float mc[3];
  world_to_cam_mean(k, m0, m1, m2, mc);
  const M3 Cc = mul(mul(k.R, C3), transpose(k.R));

  const size_t idx = (size_t)c * a.N + n;
  if (MODE == 0) a.depths[idx] = mc[2];
  const bool keep = in & (mc[2] > a.near_plane) & (mc[2] < a.far_plane);
  ewa_fwd_tail<MODE>(a, c, n, idx, keep, mc[2], persp(mc[0], mc[1], mc[2], Cc, k, a.W, a.H));
}

// ---------------------------------------------------------------- backward
// The pair a backward lane works on: dense, (blockIdx.y, lane's Gaussian)
// where its radius is positive; packed, entry e of camera_ids / gaussian_ids
// with the gradient rows at e.  Args: ProjBwdArgs or cv::BwdArgs.  The kernel
// passes its blockDim.x: read here, it is loaded through the path that allows
// non-uniform workgroups (more scalar code).
struct PairIdx {
  int c, n;
  size_t idx;
  bool valid;
};

template <class Args>
GS_INLINE PairIdx decode_pair(const Args &a, bool packed, unsigned block_dim) {
  PairIdx o;
  if (packed) {
    const int64_t e = (int64_t)blockIdx.x * block_dim + threadIdx.x;
    o.valid = e < a.nnz;
    o.c = o.valid ? (int)a.camera_ids[e] : 0;
    o.n = o.valid ? (int)a.gaussian_ids[e] : 0;
    o.idx = o.valid ? (size_t)e : 0;
  } else {
    o.c = blockIdx.y;
    o.n = blockIdx.x * block_dim + threadIdx.x;
    o.idx = (size_t)o.c * a.N + o.n;
    o.valid = (o.n < a.N) && (a.radii[o.idx] > 0);
  }
  return o;
}

struct Sym2 {
  float xx, xy, yy;
};

// Conic inverse VJP (util_kernels.py:27-61; v_conic_xy halved), then with BLUR
// the blur VJP where compensations were computed (util_kernels.py:97-144):
// the gradient of the 2D covariance before blur.
template <bool BLUR = true, class Args>
GS_INLINE Sym2 conic_blur_vjp(const Args &a, size_t idx) {
  const float *cn = a.conics + 3 * idx;
  const float ca = cn[0], cb = cn[1], cc = cn[2];
  const float *vc = a.v_conics + 3 * idx;
  const float va = vc[0], vb = 0.5f * vc[1], vcc = vc[2];
  Sym2 d;
  d.xx = -(ca * va * ca + cb * vcc * cb + 2.f * cb * vb * ca);
  d.xy = -(ca * vb * cc + cb * vb * cb + cb * vcc * cc + ca * va * cb);
  d.yy = -(cb * va * cb + cc * vcc * cc + 2.f * cc * vb * cb);
  if (BLUR && a.comps) {
    const float cp = a.comps[idx], vcp = a.v_comps[idx];
    const float det_i = ca * cc - cb * cb;
    const float Da = 0.5f * vcp / (cp + 1e-6f);
    const float oma = 1.f - cp * cp;
    d.xx += Da * (oma * ca - a.eps2d * det_i);
    d.xy += Da * (oma * cb);
    d.yy += Da * (oma * cc - a.eps2d * det_i);
  }
  return d;
}

// Perspective VJP (cam_proj.py:84-242): from the gradient d of the 2D
// covariance and (vm2x, vm2y) of means2d to v3, the gradient of the
// camera-space covariance, and vmc, that of the camera-space mean (v_depth
// not included).
//
// CLAMPED_Z picks the z-gradient of means2d, on which the two references
// differ.  The forward's means2d is the unclamped f x / z + c.  true: the
// gradient goes through the clamped Jacobian, Jxz vm2x + Jyz vm2y, as the
// Triton reference does (projection.hip).  false: it takes the unclamped
// x / z, y / z, -(fx x vm2x + fy y vm2y) / z^2, as the CUDA reference does
// (gsplat/cuda/include/Utils.cuh:521-528; projection_covar.hip).  The two
// agree wherever the screen coordinate is not clamped, so the paths differ
// only for Gaussians beyond the 15 % margin
// (tests/test_gpu_covar.py::test_covars_path_agrees_with_quats_scales_path).
template <bool CLAMPED_Z>
GS_INLINE void persp_vjp(const ProjOut &p, const Cam &k, const float (&mc)[3], const M3 &Cc,
                         const Sym2 &d, float vm2x, float vm2y, M3 &v3, float (&vmc)[3]) {
  const float dxx = d.xx, dxy = d.xy, dyy = d.yy;
  const float iz = 1.f / mc[2];
  v3.m[0][0] = p.Jxx * dxx * p.Jxx;
  v3.m[1][1] = p.Jyy * dyy * p.Jyy;
  v3.m[2][2] = p.Jxz * dxx * p.Jxz + p.Jyz * dyy * p.Jyz + 2.f * p.Jyz * dxy * p.Jxz;
  v3.m[0][1] = v3.m[1][0] = p.Jxx * dxy * p.Jyy;
  v3.m[0][2] = v3.m[2][0] = p.Jxx * dxx * p.Jxz + p.Jxx * dxy * p.Jyz;
  v3.m[1][2] = v3.m[2][1] = p.Jyy * dxy * p.Jxz + p.Jyy * dyy * p.Jyz;

  vmc[0] = p.Jxx * vm2x;
  vmc[1] = p.Jyy * vm2y;
  if (CLAMPED_Z) vmc[2] = p.Jxz * vm2x + p.Jyz * vm2y;
  else vmc[2] = -(k.fx * mc[0] * vm2x + k.fy * mc[1] * vm2y) * (iz * iz);
  const float(*cm)[3] = Cc.m;
  const float Jc_xx = p.Jxx * cm[0][0] + p.Jxz * cm[0][2];
  const float Jc_xy = p.Jxx * cm[0][1] + p.Jxz * cm[1][2];
  const float Jc_xz = p.Jxx * cm[0][2] + p.Jxz * cm[2][2];
  const float Jc_yx = p.Jyy * cm[0][1] + p.Jyz * cm[0][2];
  const float Jc_yy = p.Jyy * cm[1][1] + p.Jyz * cm[1][2];
  const float Jc_yz = p.Jyy * cm[1][2] + p.Jyz * cm[2][2];
  const float vJxx = 2.f * (dxx * Jc_xx + dxy * Jc_yx);
  const float vJxz = 2.f * (dxx * Jc_xz + dxy * Jc_yz);
  const float vJyy = 2.f * (dxy * Jc_xy + dyy * Jc_yy);
  const float vJyz = 2.f * (dxy * Jc_xz + dyy * Jc_yz);
  const float iz2 = iz * iz;
  vmc[0] += p.clamp_x ? 0.f : -vJxz * k.fx * iz2;
  vmc[1] += p.clamp_y ? 0.f : -vJyz * k.fy * iz2;
  float tmp = vJxx * p.Jxx + vJyy * p.Jyy + 2.f * (vJxz * p.Jxz + vJyz * p.Jyz);
  tmp -= p.clamp_x ? vJxz * p.Jxz : 0.f;
  tmp -= p.clamp_y ? vJyz * p.Jyz : 0.f;
  vmc[2] -= iz * tmp;
}

// ------------------------------------------------- v_viewmats reductions
// Adds the lanes' view-matrix partials vR | vt into v_viewmats [C, 4, 4]
// (zero-filled).  packed: entries are camera-major, so a wave spans one camera
// except at camera boundaries, where its lanes add their partials one by one.
// dense (the block's camera is c): wave butterfly, then LDS, then one atomic
// per block and element.  Every lane of the block must call this.
GS_INLINE void reduce_v_viewmats(float *v_viewmats, bool packed, bool valid, int c,
                                 const float (&vR)[3][3], const float (&vt)[3]) {
  if (v_viewmats && packed) {
    const int lane = threadIdx.x & 63;
    float v[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) v[i * 4 + j] = vR[i][j];
      v[i * 4 + 3] = vt[i];
    }
    const int c0 = __shfl(c, 0, 64);
    if (__ballot(valid && c != c0) == 0) {
#pragma unroll
      for (int e = 0; e < 12; ++e) v[e] = wave_sum(v[e]);
      if (lane == 0)
        for (int e = 0; e < 12; ++e)
          if (v[e] != 0.f) atomic_add_f32(v_viewmats + c0 * 16 + e, v[e]);
    } else if (valid) {
      for (int e = 0; e < 12; ++e)
        if (v[e] != 0.f) atomic_add_f32(v_viewmats + c * 16 + e, v[e]);
    }
  } else if (v_viewmats) {
    __shared__ float red[4][12];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    float v[12];
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) v[i * 4 + j] = vR[i][j];
      v[i * 4 + 3] = vt[i];
    }
#pragma unroll
    for (int e = 0; e < 12; ++e) v[e] = wave_sum(v[e]);
    if (lane == 0) {
#pragma unroll
      for (int e = 0; e < 12; ++e) red[wid][e] = v[e];
    }
    __syncthreads();
    if (threadIdx.x < 12) {
      float s = 0.f;
      for (int w = 0; w < (int)(blockDim.x >> 6); ++w) s += red[w][threadIdx.x];
      if (s != 0.f) atomic_add_f32(v_viewmats + c * 16 + threadIdx.x, s);
    }
  }
}

}  // namespace gs
