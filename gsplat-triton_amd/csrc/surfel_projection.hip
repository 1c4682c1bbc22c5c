// 2DGS (surfel) ray-splat projection for gfx950, forward and backward, dense
// and packed.  The surfel rasterizer is surfel.hip.
//
// Replaces the reference CUDA kernels (hieu1999210/gsplat-triton)
//   projection_2dgs_fused_fwd_kernel   gsplat/cuda/csrc/Projection2DGSFused.cu:17-238
//   projection_2dgs_fused_bwd_kernel   gsplat/cuda/csrc/Projection2DGSFused.cu:319-457
//     (+ compute_ray_transforms_aabb_vjp, gsplat/cuda/csrc/Projection2DGS.cuh:10-87)
//   projection_2dgs_packed_fwd_kernel  gsplat/cuda/csrc/Projection2DGSPacked.cu:17-270
//   projection_2dgs_packed_bwd_kernel  gsplat/cuda/csrc/Projection2DGSPacked.cu:274-420
// with the same algebra, on a CDNA4 mapping: one lane per (camera, surfel),
// grid (ceil(N/256), C) so the camera is a wave-uniform scalar load; the
// backward stores its gradients (atomics only when several cameras share a
// surfel).
#include "common.h"
#include "geom_adam.h"
#include "proj_math.h"  // Cam, load_view, launch_packed_scan
#include "../../include/gsplat_hip.h"

namespace gs {
namespace surfel {

struct ProjFwdArgs {
  int C, N, W, H;
  float near_plane, far_plane, radius_clip;
  const float *means, *quats, *scales, *viewmats, *Ks;
  int32_t *radii;
  float *means2d, *depths, *ray_transforms, *normals;
  // packed mode (projection_2dgs_packed_fwd, Projection2DGSPacked.cu:17-205):
  // per-block counts of kept (camera, surfel) pairs, then their exclusive
  // prefix, in (c, n) order
  int64_t *block_cnt;
  const int64_t *block_off;
  int64_t *camera_ids, *gaussian_ids;
};

// gs::load_cam with the intrinsics read in the order K[0], K[2], K[4], K[5]:
// proj_bwd_kernel (fused geometry Adam) is held to the instructions this order
// compiles to; load_K's order swaps one pair of loads.
GS_INLINE Cam load_cam_k0245(const float *__restrict__ viewmats, const float *__restrict__ Ks,
                             int c) {
  Cam k;
  load_view(k, viewmats, c);
  const float *K = Ks + 9 * c;
  k.fx = K[0];
  k.cx = K[2];
  k.fy = K[4];
  k.cy = K[5];
  return k;
}

// Camera-space surfel: mean, the two scaled tangent axes and the normal axis
// (columns of R_cw * R(q) * diag(s0, s1, 1), Projection2DGSFused.cu:164-167).
struct Frame {
  float mc[3], t0[3], t1[3], nz[3];
  M3 Rq;
};

GS_INLINE Frame surfel_frame(const Cam &k, const float *m, float4 q, float s0, float s1) {
  Frame f;
  f.Rq = quat_to_rotmat(q.x, q.y, q.z, q.w);
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    f.mc[i] = k.R.m[i][0] * m[0] + k.R.m[i][1] * m[1] + k.R.m[i][2] * m[2] + k.t[i];
    float a = 0.f, b = 0.f, c = 0.f;
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      a += k.R.m[i][j] * f.Rq.m[j][0];
      b += k.R.m[i][j] * f.Rq.m[j][1];
      c += k.R.m[i][j] * f.Rq.m[j][2];
    }
    f.t0[i] = a * s0;
    f.t1[i] = b * s1;
    f.nz[i] = c;
  }
  return f;
}

// MODE 0: dense [C, N] outputs.  MODE 1: count the kept pairs per block.
// MODE 2: write the kept pairs packed at block_off[block] + rank in block.
template <int MODE>
__global__ void __launch_bounds__(256) proj_fwd_kernel(ProjFwdArgs a) {
  const int c = blockIdx.y;
  const int n_raw = blockIdx.x * blockDim.x + threadIdx.x;
  const Cam k = load_cam_k0245(a.viewmats, a.Ks, c);
  if (MODE == 0 && n_raw >= a.N) return;
  const bool in = n_raw < a.N;
  const int n = in ? n_raw : a.N - 1;  // packed modes: every lane reaches the block scan
  const size_t idx = (size_t)c * a.N + n;
  const float4 q = *reinterpret_cast<const float4 *>(a.quats + 4 * (size_t)n);
  const float *sp = a.scales + 3 * (size_t)n;
  const Frame f = surfel_frame(k, a.means + 3 * (size_t)n, q, sp[0], sp[1]);
  if (MODE == 0) a.depths[idx] = f.mc[2];

  // rows of K * [t0 | t1 | mc] (the ray transform, M0/M1/M2 of the reference)
  float M[9];
  M[0] = k.fx * f.t0[0] + k.cx * f.t0[2];
  M[1] = k.fx * f.t1[0] + k.cx * f.t1[2];
  M[2] = k.fx * f.mc[0] + k.cx * f.mc[2];
  M[3] = k.fy * f.t0[1] + k.cy * f.t0[2];
  M[4] = k.fy * f.t1[1] + k.cy * f.t1[2];
  M[5] = k.fy * f.mc[1] + k.cy * f.mc[2];
  M[6] = f.t0[2];
  M[7] = f.t1[2];
  M[8] = f.mc[2];

  bool keep = in && !(f.mc[2] < a.near_plane || f.mc[2] > a.far_plane);
  // AABB from the (1, 1, -1) corner (Projection2DGSFused.cu:200-219)
  const float dist = M[6] * M[6] + M[7] * M[7] - M[8] * M[8];
  keep &= dist != 0.f;
  const float fi = 1.f / dist;
  const float mx = (fi * M[0]) * M[6] + (fi * M[1]) * M[7] + (-fi * M[2]) * M[8];
  const float my = (fi * M[3]) * M[6] + (fi * M[4]) * M[7] + (-fi * M[5]) * M[8];
  const float ex = mx * mx - ((fi * M[0]) * M[0] + (fi * M[1]) * M[1] + (-fi * M[2]) * M[2]);
  const float ey = my * my - ((fi * M[3]) * M[3] + (fi * M[4]) * M[4] + (-fi * M[5]) * M[5]);
  const float radius = ceilf(3.f * sqrtf(fmaxf(1e-4f, fmaxf(ex, ey))));
  keep &= radius > a.radius_clip;
  keep &= !(mx + radius <= 0.f || mx - radius >= (float)a.W || my + radius <= 0.f ||
            my - radius >= (float)a.H);

  const float sgn = -(f.nz[0] * f.mc[0] + f.nz[1] * f.mc[1] + f.nz[2] * f.mc[2]) > 0.f ? 1.f : -1.f;
  if (MODE == 0) {
    a.radii[idx] = keep ? (int32_t)radius : 0;
    *reinterpret_cast<float2 *>(a.means2d + 2 * idx) = keep ? make_float2(mx, my) : make_float2(0.f, 0.f);
    float *rt = a.ray_transforms + 9 * idx;
#pragma unroll
    for (int i = 0; i < 9; ++i) rt[i] = keep ? M[i] : 0.f;
    float *nr = a.normals + 3 * idx;
#pragma unroll
    for (int i = 0; i < 3; ++i) nr[i] = keep ? sgn * f.nz[i] : 0.f;
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
  a.radii[o] = (int32_t)radius;
  *reinterpret_cast<float2 *>(a.means2d + 2 * o) = make_float2(mx, my);
  a.depths[o] = f.mc[2];
  float *rt = a.ray_transforms + 9 * o;
#pragma unroll
  for (int i = 0; i < 9; ++i) rt[i] = M[i];
  float *nr = a.normals + 3 * o;
#pragma unroll
  for (int i = 0; i < 3; ++i) nr[i] = sgn * f.nz[i];
}

struct ProjBwdArgs {
  int C, N;
  const float *means, *quats, *scales, *viewmats, *Ks;
  const int32_t *radii;
  const float *ray_transforms, *v_means2d, *v_depths, *v_normals, *v_ray_transforms;
  float *v_means, *v_quats, *v_scales;
  int store_mode;  // C == 1: plain stores of every row; else atomics of valid rows
  // packed inputs (projection_2dgs_packed_bwd, Projection2DGSPacked.cu:274-420):
  // entry e is the pair (camera_ids[e], gaussian_ids[e]); sparse: one
  // gradient row per entry [nnz, .]
  const int64_t *camera_ids, *gaussian_ids;
  int64_t nnz;
  int sparse;
  GeomAdam ga;  // proj_bwd_kernel: the geometry Adam instead of the stores
};

// a.ga.p[0] set (ABI 33, gsplat_hip_projection_2dgs_bwd_adam; C == 1,
// dense): the geometry groups' Adam step on the lane's rows instead of
// storing v_means / v_quats / v_scales (geom_adam.h).  A runtime branch of
// the one kernel, so that the fused update consumes exactly the gradient
// values the plain backward stores (two instantiations contracted the
// algebra differently: 1 ulp in the log-scales).
__global__ void __launch_bounds__(256) proj_bwd_kernel(ProjBwdArgs a) {
  int c, n;
  size_t idx;
  bool valid;
  const bool packed = a.camera_ids != nullptr;
  if (packed) {
    const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (e >= a.nnz) return;
    c = (int)a.camera_ids[e];
    n = (int)a.gaussian_ids[e];
    idx = (size_t)e;
    valid = true;
  } else {
    c = blockIdx.y;
    n = blockIdx.x * blockDim.x + threadIdx.x;
    if (n >= a.N) return;
    idx = (size_t)c * a.N + n;
    valid = a.radii[idx] > 0;
  }
  GeomRows gr;
  const bool fuse = a.ga.p[0] != nullptr;
  const bool fuse_on = fuse && !(a.ga.skip && *a.ga.skip);
  if (fuse_on) geom_rows_load(a.ga, (size_t)n, a.scales, gr);  // in flight from here
  const Cam k = load_cam_k0245(a.viewmats, a.Ks, c);
  float vm[3] = {0.f, 0.f, 0.f}, vq[4] = {0.f, 0.f, 0.f, 0.f}, vs[3] = {0.f, 0.f, 0.f};
  if (valid) {
    const float4 q = *reinterpret_cast<const float4 *>(a.quats + 4 * (size_t)n);
    const float *sp = a.scales + 3 * (size_t)n;
    const float s0 = sp[0], s1 = sp[1];
    const Frame f = surfel_frame(k, a.means + 3 * (size_t)n, q, s0, s1);
    const float *rt = a.ray_transforms + 9 * idx;
    float V[9];
#pragma unroll
    for (int i = 0; i < 9; ++i) V[i] = a.v_ray_transforms[9 * idx + i];
    if (a.v_depths) V[8] += a.v_depths[idx];
    // means2d through the AABB formula, as the reference differentiates it
    // (Projection2DGS.cuh:25-65)
    const float gx = a.v_means2d[2 * idx], gy = a.v_means2d[2 * idx + 1];
    if (gx != 0.f || gy != 0.f) {
      float r[9];
#pragma unroll
      for (int i = 0; i < 9; ++i) r[i] = rt[i];
      const float fi = 1.f / (r[6] * r[6] + r[7] * r[7] - r[8] * r[8]);
      const float f2 = 2.f * fi * fi;
      V[0] += gx * (fi * r[6]);
      V[1] += gx * (fi * r[7]);
      V[2] += gx * (-fi * r[8]);
      V[3] += gy * (fi * r[6]);
      V[4] += gy * (fi * r[7]);
      V[5] += gy * (-fi * r[8]);
      const float e6 = fi - f2 * r[6] * r[6], e7 = fi - f2 * r[7] * r[7], e8 = fi + f2 * r[8] * r[8];
      V[6] += gx * (r[0] * e6) + gy * (r[3] * e6);
      V[7] += gx * (r[1] * e7) + gy * (r[4] * e7);
      V[8] += gx * (-r[2] * e8) + gy * (-r[5] * e8);
    }
    // d/d[t0 | t1 | mc] = K^T V (camera space), then R^T to world
    float dW[3][3];
#pragma unroll
    for (int j = 0; j < 3; ++j) {
      dW[0][j] = k.fx * V[j];
      dW[1][j] = k.fy * V[3 + j];
      dW[2][j] = k.cx * V[j] + k.cy * V[3 + j] + V[6 + j];
    }
    float vRS[3][3];  // vRS[i][j]: world-space gradient of column j
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int j = 0; j < 3; ++j)
        vRS[i][j] = k.R.m[0][i] * dW[0][j] + k.R.m[1][i] * dW[1][j] + k.R.m[2][i] * dW[2][j];
    // v_normals may be null (ABI 33: a render whose normals carry no
    // gradient): zeros through the same arithmetic
    float gn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i) gn[i] = a.v_normals ? a.v_normals[3 * idx + i] : 0.f;
    const float sgn =
        -(f.nz[0] * f.mc[0] + f.nz[1] * f.mc[1] + f.nz[2] * f.mc[2]) > 0.f ? 1.f : -1.f;
    float vtn[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
      vtn[i] = sgn * (k.R.m[0][i] * gn[0] + k.R.m[1][i] * gn[1] + k.R.m[2][i] * gn[2]);
    M3 dR;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      dR.m[i][0] = vRS[i][0] * s0;
      dR.m[i][1] = vRS[i][1] * s1;
      dR.m[i][2] = vtn[i];
    }
    quat_to_rotmat_vjp(q.x, q.y, q.z, q.w, dR, vq);
    vs[0] = vRS[0][0] * f.Rq.m[0][0] + vRS[1][0] * f.Rq.m[1][0] + vRS[2][0] * f.Rq.m[2][0];
    vs[1] = vRS[0][1] * f.Rq.m[0][1] + vRS[1][1] * f.Rq.m[1][1] + vRS[2][1] * f.Rq.m[2][1];
#pragma unroll
    for (int i = 0; i < 3; ++i) vm[i] = vRS[i][2];
  }
  // the gradients are formed once, here, for every epilogue below, each
  // rounded on its own: the fused Adam epilogue (FUSE) then consumes exactly
  // the values the plain kernel stores (without the barrier the compiler may
  // contract the algebra differently in the two instantiations)
  asm volatile("" : "+v"(vm[0]), "+v"(vm[1]), "+v"(vm[2]), "+v"(vq[0]), "+v"(vq[1]),
               "+v"(vq[2]), "+v"(vq[3]), "+v"(vs[0]), "+v"(vs[1]), "+v"(vs[2]));
  if (fuse) {
    if (fuse_on) geom_rows_update(a.ga, (size_t)n, gr, vm, vs, vq);
    return;
  }
  if (packed && a.sparse) {  // COO values, one row per packed entry
    float *o = a.v_means + 3 * idx;
    o[0] = vm[0]; o[1] = vm[1]; o[2] = vm[2];
    *reinterpret_cast<float4 *>(a.v_quats + 4 * idx) = make_float4(vq[0], vq[1], vq[2], vq[3]);
    o = a.v_scales + 3 * idx;
    o[0] = vs[0]; o[1] = vs[1]; o[2] = 0.f;
  } else if (a.store_mode) {
    float *o = a.v_means + 3 * (size_t)n;
    o[0] = vm[0]; o[1] = vm[1]; o[2] = vm[2];
    *reinterpret_cast<float4 *>(a.v_quats + 4 * (size_t)n) = make_float4(vq[0], vq[1], vq[2], vq[3]);
    o = a.v_scales + 3 * (size_t)n;
    o[0] = vs[0]; o[1] = vs[1]; o[2] = 0.f;
  } else if (valid) {
#pragma unroll
    for (int j = 0; j < 3; ++j) atomic_add_f32(a.v_means + 3 * (size_t)n + j, vm[j]);
#pragma unroll
    for (int j = 0; j < 4; ++j) atomic_add_f32(a.v_quats + 4 * (size_t)n + j, vq[j]);
    atomic_add_f32(a.v_scales + 3 * (size_t)n, vs[0]);
    atomic_add_f32(a.v_scales + 3 * (size_t)n + 1, vs[1]);
  }
}

}  // namespace surfel
}  // namespace gs

using namespace gs;
using namespace gs::surfel;

extern "C" int gsplat_hip_projection_2dgs_fwd(int C, int N, const float *means, const float *quats,
                                              const float *scales, const float *viewmats,
                                              const float *Ks, int width, int height,
                                              float near_plane, float far_plane,
                                              float radius_clip, int32_t *radii, float *means2d,
                                              float *depths, float *ray_transforms,
                                              float *normals, void *stream) {
  GS_REQUIRE(C >= 0 && N >= 0, "projection_2dgs_fwd: negative sizes C=%d N=%d", C, N);
  if (C == 0 || N == 0) return 0;
  GS_REQUIRE(means && quats && scales && viewmats && Ks && radii && means2d && depths &&
                 ray_transforms && normals,
             "projection_2dgs_fwd: null pointer argument");
  GS_REQUIRE(((uintptr_t)quats & 15) == 0 && ((uintptr_t)means2d & 7) == 0,
             "projection_2dgs_fwd: quats must be 16-B aligned, means2d 8-B aligned");
  ProjFwdArgs a{C, N, width, height, near_plane, far_plane, radius_clip, means, quats, scales,
                viewmats, Ks, radii, means2d, depths, ray_transforms, normals};
  hipLaunchKernelGGL(proj_fwd_kernel<0>, dim3((N + 255) / 256, C), dim3(256), 0,
                     (hipStream_t)stream, a);
  GS_CHECK_LAUNCH("projection_2dgs_fwd");
  return 0;
}

extern "C" int gsplat_hip_projection_2dgs_bwd(
    int C, int N, const float *means, const float *quats, const float *scales,
    const float *viewmats, const float *Ks, int width, int height, const int32_t *radii,
    const float *ray_transforms, const float *v_means2d, const float *v_depths,
    const float *v_normals, const float *v_ray_transforms, float *v_means, float *v_quats,
    float *v_scales, float *v_viewmats, void *stream) {
  (void)width;
  (void)height;
  GS_REQUIRE(C >= 0 && N >= 0, "projection_2dgs_bwd: negative sizes C=%d N=%d", C, N);
  hipStream_t st = (hipStream_t)stream;
  // the reference allocates v_viewmats but its kernel never writes it
  // (Projection2DGSFused.cu:319-457): zeros
  if (v_viewmats && C > 0) GS_HIP(gs::zero_async(v_viewmats, sizeof(float) * 16 * C, st));
  if (N == 0) return 0;
  const int store_mode = (C == 1);
  if (!store_mode) {
    GS_HIP(gs::zero_async(v_means, sizeof(float) * 3 * N, st));
    GS_HIP(gs::zero_async(v_quats, sizeof(float) * 4 * N, st));
    GS_HIP(gs::zero_async(v_scales, sizeof(float) * 3 * N, st));
  }
  if (C == 0) return 0;
  GS_REQUIRE(means && quats && scales && viewmats && Ks && radii && ray_transforms &&
                 v_means2d && v_ray_transforms && v_means && v_quats && v_scales,
             "projection_2dgs_bwd: null pointer argument");
  GS_REQUIRE(((uintptr_t)quats & 15) == 0 && ((uintptr_t)v_quats & 15) == 0,
             "projection_2dgs_bwd: quats / v_quats must be 16-B aligned");
  ProjBwdArgs a{C, N, means, quats, scales, viewmats, Ks, radii, ray_transforms, v_means2d,
                v_depths, v_normals, v_ray_transforms, v_means, v_quats, v_scales, store_mode};
  hipLaunchKernelGGL(proj_bwd_kernel, dim3((N + 255) / 256, C), dim3(256), 0, st, a);
  GS_CHECK_LAUNCH("projection_2dgs_bwd");
  return 0;
}

// gsplat_hip_projection_2dgs_bwd with the geometry groups' Adam step fused in
// (ABI 33; geom_adam.h, as gsplat_hip_projection_bwd_adam for 3DGS): one
// camera; params / exp_avgs / exp_avg_sqs are [means, log_scales, quats,
// logits]; lrs[4] with the 1-based step, or hyper_device f32[8]; skip_device
// may be NULL.  No gradient is stored.
extern "C" int gsplat_hip_projection_2dgs_bwd_adam(
    int N, const float *means, const float *quats, const float *scales, const float *viewmats,
    const float *Ks, const int32_t *radii, const float *ray_transforms, const float *v_means2d,
    const float *v_depths, const float *v_normals, const float *v_ray_transforms,
    const float *v_dirs, const float *v_opac, const float *opac, float *const *params,
    float *const *exp_avgs, float *const *exp_avg_sqs, const float *lrs, float beta1,
    float beta2, float eps, int step, const float *hyper_device, const int32_t *skip_device,
    void *stream) {
  GS_REQUIRE(N >= 0, "projection_2dgs_bwd_adam: negative N=%d", N);
  if (N == 0) return 0;
  GS_REQUIRE(means && quats && scales && viewmats && Ks && radii && ray_transforms &&
                 v_means2d && v_ray_transforms,
             "projection_2dgs_bwd_adam: null pointer argument");
  GS_REQUIRE(((uintptr_t)quats & 15) == 0, "projection_2dgs_bwd_adam: quats must be 16-B aligned");
  GeomAdam ga;
  if (int e = geom_adam_setup(ga, params, exp_avgs, exp_avg_sqs, lrs, beta1, beta2, eps, step,
                              hyper_device, skip_device, v_dirs, v_opac, opac,
                              "projection_2dgs_bwd_adam"))
    return e;
  ProjBwdArgs a{1, N, means, quats, scales, viewmats, Ks, radii, ray_transforms, v_means2d,
                v_depths, v_normals, v_ray_transforms, nullptr, nullptr, nullptr, 1};
  a.ga = ga;
  hipLaunchKernelGGL(proj_bwd_kernel, dim3((N + 255) / 256, 1), dim3(256), 0,
                     (hipStream_t)stream, a);
  GS_CHECK_LAUNCH("projection_2dgs_bwd_adam");
  return 0;
}

// ------------------------------------------------------------------ packed --
// projection_2dgs_packed_fwd (gsplat/cuda/csrc/Projection2DGSPacked.cu:17-270):
// a counting pass, a scan of the per-block counts and a pass that recomputes
// and writes the kept (camera, surfel) pairs in (camera, surfel) order.
extern "C" int64_t gsplat_hip_projection_2dgs_packed_workspace_bytes(int C, int N) {
  const int64_t nb = (int64_t)C * ((N + 255) / 256);
  return (nb + 1) * (int64_t)sizeof(int64_t);
}

extern "C" int gsplat_hip_projection_2dgs_packed_count(
    int C, int N, const float *means, const float *quats, const float *scales,
    const float *viewmats, const float *Ks, int width, int height, float near_plane,
    float far_plane, float radius_clip, void *workspace, int64_t *nnz_device, void *stream) {
  GS_REQUIRE(C >= 0 && N >= 0, "projection_2dgs_packed_count: negative sizes C=%d N=%d", C, N);
  hipStream_t st = (hipStream_t)stream;
  if (C == 0 || N == 0) {
    GS_HIP(gs::zero_async(nnz_device, sizeof(int64_t), st));
    return 0;
  }
  GS_REQUIRE(means && quats && scales && viewmats && Ks && workspace && nnz_device,
             "projection_2dgs_packed_count: null pointer argument");
  GS_REQUIRE(((uintptr_t)quats & 15) == 0,
             "projection_2dgs_packed_count: quats must be 16-B aligned");
  ProjFwdArgs a{C, N, width, height, near_plane, far_plane, radius_clip, means, quats, scales,
                viewmats, Ks};
  a.block_cnt = reinterpret_cast<int64_t *>(workspace);
  const dim3 grid((N + 255) / 256, C);
  hipLaunchKernelGGL(proj_fwd_kernel<1>, grid, dim3(256), 0, st, a);
  gs::launch_packed_scan((int64_t)grid.x * grid.y, a.block_cnt, nnz_device, st);
  GS_CHECK_LAUNCH("projection_2dgs_packed_count");
  return 0;
}

extern "C" int gsplat_hip_projection_2dgs_packed_fwd(
    int C, int N, const float *means, const float *quats, const float *scales,
    const float *viewmats, const float *Ks, int width, int height, float near_plane,
    float far_plane, float radius_clip, const void *workspace, int64_t *camera_ids,
    int64_t *gaussian_ids, int32_t *radii, float *means2d, float *depths, float *ray_transforms,
    float *normals, void *stream) {
  GS_REQUIRE(C >= 0 && N >= 0, "projection_2dgs_packed_fwd: negative sizes C=%d N=%d", C, N);
  if (C == 0 || N == 0) return 0;
  GS_REQUIRE(means && quats && scales && viewmats && Ks && workspace && camera_ids &&
                 gaussian_ids && radii && means2d && depths && ray_transforms && normals,
             "projection_2dgs_packed_fwd: null pointer argument");
  GS_REQUIRE(((uintptr_t)quats & 15) == 0 && ((uintptr_t)means2d & 7) == 0,
             "projection_2dgs_packed_fwd: quats must be 16-B aligned, means2d 8-B aligned");
  ProjFwdArgs a{C, N, width, height, near_plane, far_plane, radius_clip, means, quats, scales,
                viewmats, Ks, radii, means2d, depths, ray_transforms, normals};
  a.block_off = reinterpret_cast<const int64_t *>(workspace);
  a.camera_ids = camera_ids;
  a.gaussian_ids = gaussian_ids;
  hipLaunchKernelGGL(proj_fwd_kernel<2>, dim3((N + 255) / 256, C), dim3(256), 0,
                     (hipStream_t)stream, a);
  GS_CHECK_LAUNCH("projection_2dgs_packed_fwd");
  return 0;
}

// projection_2dgs_packed_bwd (Projection2DGSPacked.cu:274-420): one lane per
// packed entry; dense [N, .] gradients by atomics, or (sparse_grad) one row
// per entry for the COO gradients of _wrapper.py:1529-1570.  v_viewmats, as
// in the reference, is not differentiated (zeros).
extern "C" int gsplat_hip_projection_2dgs_packed_bwd(
    int C, int N, int64_t nnz, const float *means, const float *quats, const float *scales,
    const float *viewmats, const float *Ks, int width, int height, const int64_t *camera_ids,
    const int64_t *gaussian_ids, const float *ray_transforms, const float *v_means2d,
    const float *v_depths, const float *v_normals, const float *v_ray_transforms,
    int sparse_grad, float *v_means, float *v_quats, float *v_scales, float *v_viewmats,
    void *stream) {
  (void)width;
  (void)height;
  GS_REQUIRE(C >= 0 && N >= 0 && nnz >= 0, "projection_2dgs_packed_bwd: negative sizes");
  hipStream_t st = (hipStream_t)stream;
  if (v_viewmats && C > 0) GS_HIP(gs::zero_async(v_viewmats, sizeof(float) * 16 * C, st));
  if (!sparse_grad && N > 0) {
    GS_HIP(gs::zero_async(v_means, sizeof(float) * 3 * N, st));
    GS_HIP(gs::zero_async(v_quats, sizeof(float) * 4 * N, st));
    GS_HIP(gs::zero_async(v_scales, sizeof(float) * 3 * N, st));
  }
  if (nnz == 0) return 0;
  GS_REQUIRE(means && quats && scales && viewmats && Ks && camera_ids && gaussian_ids &&
                 ray_transforms && v_means2d && v_normals && v_ray_transforms && v_means &&
                 v_quats && v_scales,
             "projection_2dgs_packed_bwd: null pointer argument");
  GS_REQUIRE(((uintptr_t)quats & 15) == 0 && ((uintptr_t)v_quats & 15) == 0,
             "projection_2dgs_packed_bwd: quats / v_quats must be 16-B aligned");
  ProjBwdArgs a{C, N, means, quats, scales, viewmats, Ks, nullptr, ray_transforms, v_means2d,
                v_depths, v_normals, v_ray_transforms, v_means, v_quats, v_scales, 0};
  a.camera_ids = camera_ids;
  a.gaussian_ids = gaussian_ids;
  a.nnz = nnz;
  a.sparse = sparse_grad;
  hipLaunchKernelGGL(proj_bwd_kernel, dim3((unsigned)((nnz + 255) / 256)), dim3(256), 0, st, a);
  GS_CHECK_LAUNCH("projection_2dgs_packed_bwd");
  return 0;
}
