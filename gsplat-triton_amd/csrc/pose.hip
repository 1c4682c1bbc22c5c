// Camera pose refinement for the 3DGS trainer (ABI 38), for gfx950.
//
// The reference's CameraOptModule (examples/utils.py): per training image a
// row e = (dx[3], d6[6]), zero-initialised; R = rotation_6d_to_matrix(d6 +
// identity) (Gram-Schmidt, rows b1, b2, b3), T = [[R, dx], [0, 1]], adjusted
// camera-to-world c2w' = c2w T.  The trainer holds view matrices, so the step
// uses viewmat' = T^-1 viewmat with T^-1 = [[R^T, -R^T dx], [0, 1]]: no
// general inverse on the device.
//
//   pose_apply_kernel     the step's adjusted view matrix (one lane)
//   pose_bwd_adam_kernel  ordered sum of the projection backward's per-block
//                         partials, the chain back to (dx, d6), dense Adam
//                         with L2 weight decay over the whole table
//   pose_adjust_*_kernel  c2w T and its VJP for users' own trainers
#include "common.h"
#include "../../include/gsplat_hip.h"

namespace gs {

constexpr float kPoseEps = 1e-12f;  // F.normalize's clamp

// rotation_6d_to_matrix(d6 + (1,0,0,0,1,0)): rows b1, b2, b3, and what the
// VJP reuses.  A zero d6 gives the identity exactly.
struct Rot6 {
  float b[3][3];
  float a2[3];
  float d;        // b1 . a2
  float l1, l2;   // |a1|, |a2 - d b1|
};

GS_INLINE float dot3(const float *x, const float *y) {
  return x[0] * y[0] + x[1] * y[1] + x[2] * y[2];
}

GS_INLINE void cross3(const float *x, const float *y, float *o) {
  o[0] = x[1] * y[2] - x[2] * y[1];
  o[1] = x[2] * y[0] - x[0] * y[2];
  o[2] = x[0] * y[1] - x[1] * y[0];
}

GS_INLINE void rot6_fwd(const float *d6, Rot6 &r) {
  const float a1[3] = {d6[0] + 1.f, d6[1], d6[2]};
  r.a2[0] = d6[3];
  r.a2[1] = d6[4] + 1.f;
  r.a2[2] = d6[5];
  r.l1 = sqrtf(dot3(a1, a1));
  const float n1 = fmaxf(r.l1, kPoseEps);
#pragma unroll
  for (int j = 0; j < 3; ++j) r.b[0][j] = a1[j] / n1;
  r.d = dot3(r.b[0], r.a2);
  float u[3];
#pragma unroll
  for (int j = 0; j < 3; ++j) u[j] = r.a2[j] - r.d * r.b[0][j];
  r.l2 = sqrtf(dot3(u, u));
  const float n2 = fmaxf(r.l2, kPoseEps);
#pragma unroll
  for (int j = 0; j < 3; ++j) r.b[1][j] = u[j] / n2;
  cross3(r.b[0], r.b[1], r.b[2]);
}

// x / max(|x|, eps): VJP given the normalised vector b and |x|
GS_INLINE void normalize_vjp(const float *b, float len, const float *vb, float *vx) {
  const float inv = 1.f / fmaxf(len, kPoseEps);
  const float s = len > kPoseEps ? dot3(b, vb) : 0.f;
#pragma unroll
  for (int j = 0; j < 3; ++j) vx[j] = (vb[j] - s * b[j]) * inv;
}

// vR[k][j] = dL/dR[k][j] (rows b1, b2, b3)  ->  v_d6[6]
GS_INLINE void rot6_vjp(const Rot6 &r, const float (&vR)[3][3], float *v_d6) {
  float vb1[3], vb2[3], t[3];
  // b3 = b1 x b2
  cross3(r.b[1], vR[2], t);
#pragma unroll
  for (int j = 0; j < 3; ++j) vb1[j] = vR[0][j] + t[j];
  cross3(vR[2], r.b[0], t);
#pragma unroll
  for (int j = 0; j < 3; ++j) vb2[j] = vR[1][j] + t[j];
  // b2 = normalize(u), u = a2 - d b1, d = b1 . a2
  float vu[3];
  normalize_vjp(r.b[1], r.l2, vb2, vu);
  const float vd = -dot3(vu, r.b[0]);
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    v_d6[3 + j] = vu[j] + vd * r.b[0][j];
    vb1[j] += vd * r.a2[j] - r.d * vu[j];
  }
  // b1 = normalize(a1)
  normalize_vjp(r.b[0], r.l1, vb1, v_d6);
}

// out = T(e)^-1 V for an affine V (bottom row copied): the rotation block is
// R^T V_R, the translation R^T (V_t - dx).  With e = 0 every product is by an
// exact 1 or 0 and V_t - 0 is V_t: out is V bit for bit.
GS_INLINE void pose_inv_apply(const float *e, const float *V, float *out) {
  Rot6 r;
  rot6_fwd(e + 3, r);
  const float d[3] = {V[3] - e[0], V[7] - e[1], V[11] - e[2]};
#pragma unroll
  for (int i = 0; i < 3; ++i) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      out[4 * i + j] = r.b[0][i] * V[j] + r.b[1][i] * V[4 + j] + r.b[2][i] * V[8 + j];
    out[4 * i + 3] = r.b[0][i] * d[0] + r.b[1][i] * d[1] + r.b[2][i] * d[2];
  }
#pragma unroll
  for (int j = 0; j < 4; ++j) out[12 + j] = V[12 + j];
}

GS_INLINE int64_t pose_row(const int64_t *cam, int n_images) {
  const int64_t c = cam[0];
  return c < 0 ? 0 : (c >= n_images ? (int64_t)n_images - 1 : c);
}

// the base view matrix with the fixed perturbation applied (pose_noise)
GS_INLINE void pose_base(const float *base, const float *noise, int64_t ci, float *V1) {
  float V[16];
#pragma unroll
  for (int k = 0; k < 16; ++k) V[k] = base[k];
  if (noise) {
    pose_inv_apply(noise + 9 * ci, V, V1);
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) V1[k] = V[k];
  }
}

__global__ void __launch_bounds__(64) pose_apply_kernel(
    const float *__restrict__ base, const int64_t *__restrict__ cam, int n_images,
    const float *__restrict__ embeds, const float *__restrict__ noise,
    float *__restrict__ viewmat_out, float *__restrict__ c2w_out) {
  if (threadIdx.x != 0) return;
  const int64_t ci = pose_row(cam, n_images);
  float V1[16], Vo[16];
  pose_base(base, noise, ci, V1);
  if (embeds) {
    pose_inv_apply(embeds + 9 * ci, V1, Vo);
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) Vo[k] = V1[k];
  }
#pragma unroll
  for (int k = 0; k < 16; ++k) viewmat_out[k] = Vo[k];
  if (c2w_out) {  // the rigid inverse [R'^T, -R'^T t']
#pragma unroll
    for (int i = 0; i < 3; ++i) {
#pragma unroll
      for (int j = 0; j < 3; ++j) c2w_out[4 * i + j] = Vo[4 * j + i];
      c2w_out[4 * i + 3] = -(Vo[i] * Vo[3] + Vo[4 + i] * Vo[7] + Vo[8 + i] * Vo[11]);
    }
    c2w_out[12] = 0.f; c2w_out[13] = 0.f; c2w_out[14] = 0.f; c2w_out[15] = 1.f;
  }
}

struct PoseBwdArgs {
  const float *ws;  // [nblocks][16]: vR|vt as [3][4], then sum v_dirs, then 0
  int nblocks, n_images;
  const float *base;
  const int64_t *cam;
  float *embeds;
  const float *noise;
  float *m, *v;
  float ss, ib;
  const float *hyper;   // device (ss, ib) of a captured step, or null
  const int32_t *skip;  // device flag: non-zero = void step
  float b1, b2, eps, wd;
};

__global__ void __launch_bounds__(1024) pose_bwd_adam_kernel(PoseBwdArgs a) {
  __shared__ float part[64][16];
  __shared__ float tot[16];
  __shared__ float grad[9];
  if (a.skip && *a.skip) return;  // uniform: before any barrier
  const int tid = threadIdx.x;
  {  // rows r, r + 64, ... of column c, then the 64 partials in order: the
     // same sequence of additions for the same workspace
    const int r = tid >> 4, c = tid & 15;
    float s = 0.f;
#pragma unroll 4
    for (int row = r; row < a.nblocks; row += 64) s += a.ws[(size_t)row * 16 + c];
    part[r][c] = s;
  }
  __syncthreads();
  if (tid < 16) {
    float t = 0.f;
    for (int r = 0; r < 64; ++r) t += part[r][tid];
    tot[tid] = t;
  }
  __syncthreads();
  const int64_t ci = pose_row(a.cam, a.n_images);
  if (tid == 0) {
    float V1[16];
    pose_base(a.base, a.noise, ci, V1);
    const float *e = a.embeds + 9 * ci;
    Rot6 r;
    rot6_fwd(e + 3, r);
    const float d[3] = {V1[3] - e[0], V1[7] - e[1], V1[11] - e[2]};
    // viewmat' = [R^T R1, R^T (t1 - dx)]: dL/dR[k][i] = sum_j vR'[i][j] R1[k][j]
    // + vt'[i] (t1 - dx)[k]
    float vR[3][3];
#pragma unroll
    for (int k = 0; k < 3; ++k)
#pragma unroll
      for (int i = 0; i < 3; ++i)
        vR[k][i] = tot[4 * i] * V1[4 * k] + tot[4 * i + 1] * V1[4 * k + 1] +
                   tot[4 * i + 2] * V1[4 * k + 2] + tot[4 * i + 3] * d[k];
    // dx: through t' = R^T (t1 - dx), and through the camera centre the SH
    // directions use, campos = R1^T dx + const with v_campos = -sum v_dirs
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      const float through_t = r.b[k][0] * tot[3] + r.b[k][1] * tot[7] + r.b[k][2] * tot[11];
      const float through_c = V1[4 * k] * tot[12] + V1[4 * k + 1] * tot[13] +
                              V1[4 * k + 2] * tot[14];
      grad[k] = -through_t - through_c;
    }
    float v_d6[6];
    rot6_vjp(r, vR, v_d6);
#pragma unroll
    for (int k = 0; k < 6; ++k) grad[3 + k] = v_d6[k];
  }
  __syncthreads();
  const float ss = a.hyper ? a.hyper[0] : a.ss, ib = a.hyper ? a.hyper[1] : a.ib;
  const int64_t total = (int64_t)a.n_images * 9;
  for (int64_t i = tid; i < total; i += 1024) {
    const int64_t row = i / 9;
    const int k = (int)(i - row * 9);
    float p = a.embeds[i], m = a.m[i], v = a.v[i];
    // torch.optim.Adam(weight_decay): g += wd * w, for every row
    const float g = __fmaf_rn(a.wd, p, row == ci ? grad[k] : 0.f);
    adam_update(p, g, m, v, a.b1, a.b2, a.eps, ss, ib);
    a.embeds[i] = p;
    a.m[i] = m;
    a.v[i] = v;
  }
}

// c2w' = c2w T(e), one lane per matrix (all four rows of c2w are used)
__global__ void __launch_bounds__(64) pose_adjust_fwd_kernel(int64_t B,
                                                             const float *__restrict__ c2w,
                                                             const float *__restrict__ deltas,
                                                             float *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= B) return;
  const float *C = c2w + 16 * i, *e = deltas + 9 * i;
  Rot6 r;
  rot6_fwd(e + 3, r);
  float *o = out + 16 * i;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      o[4 * q + j] = C[4 * q] * r.b[0][j] + C[4 * q + 1] * r.b[1][j] + C[4 * q + 2] * r.b[2][j];
    o[4 * q + 3] = C[4 * q + 3] + (C[4 * q] * e[0] + C[4 * q + 1] * e[1] + C[4 * q + 2] * e[2]);
  }
}

__global__ void __launch_bounds__(64) pose_adjust_bwd_kernel(int64_t B,
                                                             const float *__restrict__ c2w,
                                                             const float *__restrict__ deltas,
                                                             const float *__restrict__ v_out,
                                                             float *__restrict__ v_deltas) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= B) return;
  const float *C = c2w + 16 * i, *e = deltas + 9 * i, *g = v_out + 16 * i;
  Rot6 r;
  rot6_fwd(e + 3, r);
  float vR[3][3];
  float *o = v_deltas + 9 * i;
#pragma unroll
  for (int k = 0; k < 3; ++k) {
#pragma unroll
    for (int j = 0; j < 3; ++j)
      vR[k][j] = C[k] * g[j] + C[4 + k] * g[4 + j] + C[8 + k] * g[8 + j] + C[12 + k] * g[12 + j];
    o[k] = C[k] * g[3] + C[4 + k] * g[7] + C[8 + k] * g[11] + C[12 + k] * g[15];
  }
  float v_d6[6];
  rot6_vjp(r, vR, v_d6);
#pragma unroll
  for (int k = 0; k < 6; ++k) o[3 + k] = v_d6[k];
}

}  // namespace gs

using namespace gs;

extern "C" int64_t gsplat_hip_pose_workspace_bytes(int N) {
  const int64_t nb = N > 0 ? ((int64_t)N + 255) / 256 : 0;
  return (nb > 0 ? nb : 1) * 16 * (int64_t)sizeof(float);
}

extern "C" int gsplat_hip_pose_apply(int n_images, const float *base_viewmat,
                                     const int64_t *cam_index, const float *embeds,
                                     const float *noise, float *viewmat_out, float *camtoworld_out,
                                     void *stream) {
  GS_REQUIRE(n_images >= 1, "pose_apply: n_images=%d", n_images);
  GS_REQUIRE(base_viewmat && cam_index && viewmat_out, "pose_apply: null pointer argument");
  GS_REQUIRE(viewmat_out != base_viewmat, "pose_apply: viewmat_out must not alias the base");
  hipLaunchKernelGGL(pose_apply_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, base_viewmat,
                     cam_index, n_images, embeds, noise, viewmat_out, camtoworld_out);
  GS_CHECK_LAUNCH("pose_apply");
  return 0;
}

extern "C" int gsplat_hip_pose_bwd_adam(int n_images, int N, const void *workspace,
                                        const float *base_viewmat, const int64_t *cam_index,
                                        float *embeds, const float *noise, float *exp_avg,
                                        float *exp_avg_sq, float lr, float beta1, float beta2,
                                        float eps, float weight_decay, int step,
                                        const float *hyper_device, const int32_t *skip_device,
                                        void *stream) {
  GS_REQUIRE(n_images >= 1 && N >= 0, "pose_bwd_adam: n_images=%d N=%d", n_images, N);
  GS_REQUIRE(base_viewmat && cam_index && embeds && exp_avg && exp_avg_sq,
             "pose_bwd_adam: null pointer argument");
  GS_REQUIRE(workspace || N == 0, "pose_bwd_adam: null workspace");
  GS_REQUIRE(hyper_device || step >= 1, "pose_bwd_adam: step >= 1, or hyper");
  PoseBwdArgs a{};
  a.ws = reinterpret_cast<const float *>(workspace);
  a.nblocks = (N + 255) / 256;
  a.n_images = n_images;
  a.base = base_viewmat;
  a.cam = cam_index;
  a.embeds = embeds;
  a.noise = noise;
  a.m = exp_avg;
  a.v = exp_avg_sq;
  a.hyper = hyper_device;
  a.skip = skip_device;
  a.b1 = beta1;
  a.b2 = beta2;
  a.eps = eps;
  a.wd = weight_decay;
  if (!hyper_device) {  // gsplat_hip_adam_step's host arithmetic
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    a.ss = (float)(lr / bc1);
    a.ib = (float)(1.0 / sqrt(bc2));
  }
  hipLaunchKernelGGL(pose_bwd_adam_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, a);
  GS_CHECK_LAUNCH("pose_bwd_adam");
  return 0;
}

extern "C" int gsplat_hip_pose_adjust_fwd(int64_t B, const float *camtoworlds,
                                          const float *deltas, float *out, void *stream) {
  GS_REQUIRE(B >= 0, "pose_adjust_fwd: negative B");
  if (B == 0) return 0;
  GS_REQUIRE(camtoworlds && deltas && out, "pose_adjust_fwd: null pointer argument");
  hipLaunchKernelGGL(pose_adjust_fwd_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0,
                     (hipStream_t)stream, B, camtoworlds, deltas, out);
  GS_CHECK_LAUNCH("pose_adjust_fwd");
  return 0;
}

extern "C" int gsplat_hip_pose_adjust_bwd(int64_t B, const float *camtoworlds,
                                          const float *deltas, const float *v_out,
                                          float *v_deltas, void *stream) {
  GS_REQUIRE(B >= 0, "pose_adjust_bwd: negative B");
  if (B == 0) return 0;
  GS_REQUIRE(camtoworlds && deltas && v_out && v_deltas, "pose_adjust_bwd: null pointer argument");
  hipLaunchKernelGGL(pose_adjust_bwd_kernel, dim3((unsigned)((B + 63) / 64)), dim3(64), 0,
                     (hipStream_t)stream, B, camtoworlds, deltas, v_out, v_deltas);
  GS_CHECK_LAUNCH("pose_adjust_bwd");
  return 0;
}
