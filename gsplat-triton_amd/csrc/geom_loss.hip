// The 2DGS trainer's geometry terms (simple_trainer_2dgs.py: normal_loss,
// dist_loss), fused: per camera c and pixel p
//
//   L = normal_lambda * mean(1 - <R_c n_cam(p), alpha(p) n_d(p)>)
//     + dist_lambda   * mean(distort(p))
//
// with n_d the normal of the rendered depth (aux_ops.hip
// depth_to_normal_kernel: central differences of the back-projected
// 4-neighbourhood, normalised with the 1e-12 floor, zero on the one-pixel
// border) formed in registers -- no [H,W,3] image of it reaches HBM.  Both
// means run over all C*H*W pixels.  alpha is a constant (no gradient), as in
// the reference trainer.
//
// The differences are taken between z*dir of the neighbours: the camera
// origin cancels in p[y+1] - p[y-1], so it is never added (the same
// formula, without its rounding).
//
// Forward: one lane per pixel, the two sums reduced in a fixed order (wave
// butterfly, the workgroup's four waves in index order, one partial pair per
// workgroup), then one workgroup sums the partials in index order in double.
// No atomics, no pre-zeroed buffer.
// Backward: one lane per pixel, every output element written exactly once.
// The depth of q enters the normals of q's four neighbours; the lane of q
// recomputes each interior neighbour's a x b and the VJP of the floored
// normalisation and the cross product (plain gathers over the 13-point
// diamond: its reads are L2 / L1 hits), and keeps the component along q's
// ray.  No atomics, no zero fill.
#include "common.h"

namespace gs {
namespace geomk {

struct Cam {
  float R[9], fx, fy, cx, cy;
};

GS_INLINE Cam load_cam(const float *__restrict__ c2w, const float *__restrict__ K) {
  Cam m;
#pragma unroll
  for (int i = 0; i < 3; ++i)
#pragma unroll
    for (int j = 0; j < 3; ++j) m.R[3 * i + j] = c2w[4 * i + j];
  m.fx = K[0], m.fy = K[4], m.cx = K[2], m.cy = K[5];
  return m;
}

// the ray direction of pixel (x, y) in world space (depth_to_points)
GS_INLINE void ray_dir(const Cam &m, int x, int y, int z_depth, float d[3]) {
  const float dx = ((float)x - m.cx + 0.5f) / m.fx, dy = ((float)y - m.cy + 0.5f) / m.fy;
#pragma unroll
  for (int i = 0; i < 3; ++i) d[i] = m.R[3 * i] * dx + m.R[3 * i + 1] * dy + m.R[3 * i + 2];
  if (!z_depth) {
    const float n = fmaxf(sqrtf(d[0] * d[0] + d[1] * d[1] + d[2] * d[2]), 1e-12f);
#pragma unroll
    for (int i = 0; i < 3; ++i) d[i] /= n;
  }
}

GS_INLINE void cross3(const float a[3], const float b[3], float n[3]) {
  n[0] = a[1] * b[2] - a[2] * b[1];
  n[1] = a[2] * b[0] - a[0] * b[2];
  n[2] = a[0] * b[1] - a[1] * b[0];
}

// a = p[y+1,x] - p[y-1,x], b = p[y,x+1] - p[y,x-1] of an interior pixel
// (dep: the camera's depth image, pixel stride ps)
GS_INLINE void diffs(const Cam &m, const float *__restrict__ dep, int64_t ps, int W, int x, int y,
                     int z_depth, float a[3], float b[3]) {
  float dd[3], du[3], dr[3], dl[3];
  ray_dir(m, x, y + 1, z_depth, dd);
  ray_dir(m, x, y - 1, z_depth, du);
  ray_dir(m, x + 1, y, z_depth, dr);
  ray_dir(m, x - 1, y, z_depth, dl);
  const float zd = dep[((int64_t)(y + 1) * W + x) * ps], zu = dep[((int64_t)(y - 1) * W + x) * ps];
  const float zr = dep[((int64_t)y * W + x + 1) * ps], zl = dep[((int64_t)y * W + x - 1) * ps];
#pragma unroll
  for (int i = 0; i < 3; ++i) {
    a[i] = zd * dd[i] - zu * du[i];
    b[i] = zr * dr[i] - zl * dl[i];
  }
}

// the normal image in world space: R n, or n itself (already rotated)
GS_INLINE void world_normal(const Cam &m, const float *__restrict__ n, int world, float w[3]) {
  const float x = n[0], y = n[1], z = n[2];
  if (world) {
    w[0] = x, w[1] = y, w[2] = z;
    return;
  }
#pragma unroll
  for (int i = 0; i < 3; ++i) w[i] = m.R[3 * i] * x + m.R[3 * i + 1] * y + m.R[3 * i + 2] * z;
}

__global__ void __launch_bounds__(256)
fwd_kernel(int C, int H, int W, const float *__restrict__ normals,
           const float *__restrict__ depths, int64_t ps, const float *__restrict__ alphas,
           const float *__restrict__ distort, const float *__restrict__ camtoworlds,
           const float *__restrict__ Ks, int z_depth, int world, int do_n, int do_d,
           float *__restrict__ partials) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t HW = (int64_t)H * W;
  float tn = 0.f, td = 0.f;
  if (i < C * HW) {
    if (do_d) td = distort[i];
    if (do_n) {
      tn = 1.f;  // the border: n_d = 0
      const int c = (int)(i / HW);
      const int64_t r = i - c * HW;
      const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
      if (x > 0 && y > 0 && x < W - 1 && y < H - 1) {
        const Cam m = load_cam(camtoworlds + 16 * c, Ks + 9 * c);
        float a[3], b[3], n[3], w[3];
        diffs(m, depths + c * HW * ps, ps, W, x, y, z_depth, a, b);
        cross3(a, b, n);
        const float l = fmaxf(sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), 1e-12f);
        world_normal(m, normals + 3 * i, world, w);
        tn = 1.f - alphas[i] * ((w[0] * n[0] + w[1] * n[1] + w[2] * n[2]) / l);
      }
    }
  }
  tn = wave_sum(tn);
  td = wave_sum(td);
  __shared__ float s[2][4];
  const int wave = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) s[0][wave] = tn, s[1][wave] = td;
  __syncthreads();
  if (threadIdx.x == 0) {
    partials[2 * (int64_t)blockIdx.x] = ((s[0][0] + s[0][1]) + s[0][2]) + s[0][3];
    partials[2 * (int64_t)blockIdx.x + 1] = ((s[1][0] + s[1][1]) + s[1][2]) + s[1][3];
  }
}

GS_INLINE double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

// one workgroup: lane t sums partials t, t + 256, ... in that order (double),
// then the wave butterfly and the four waves in index order
__global__ void __launch_bounds__(256)
finish_kernel(int64_t n_partials, const float *__restrict__ partials, double inv_p, float nl,
              float dl, float *__restrict__ out) {
  double sn = 0.0, sd = 0.0;
  for (int64_t k = threadIdx.x; k < n_partials; k += 256) {
    const float2 v = reinterpret_cast<const float2 *>(partials)[k];
    sn += (double)v.x;
    sd += (double)v.y;
  }
  sn = wave_sum_f64(sn);
  sd = wave_sum_f64(sd);
  __shared__ double s[2][4];
  if ((threadIdx.x & 63) == 0) s[0][threadIdx.x >> 6] = sn, s[1][threadIdx.x >> 6] = sd;
  __syncthreads();
  if (threadIdx.x == 0) {
    sn = ((s[0][0] + s[0][1]) + s[0][2]) + s[0][3];
    sd = ((s[1][0] + s[1][1]) + s[1][2]) + s[1][3];
    const float mn = (float)(sn * inv_p), md = (float)(sd * inv_p);
    out[0] = nl * mn + dl * md;
    out[1] = mn;
    out[2] = md;
  }
}

// the gradient of neighbour m = (mx, my)'s normal term with respect to its
// a (which = 0) or b (which = 1), times `sign`, added to vp; sc = -g nl / P
GS_INLINE void neighbour_vjp(const Cam &cam, const float *__restrict__ dep, int64_t ps,
                             const float *__restrict__ normals, const float *__restrict__ alphas,
                             int H, int W, int mx, int my, int z_depth, int world, float sc,
                             int which, float sign, float vp[3]) {
  if (mx <= 0 || my <= 0 || mx >= W - 1 || my >= H - 1) return;  // n_d(m) = 0: no gradient
  const int64_t mi = (int64_t)my * W + mx;
  const float am = alphas[mi];
  if (am == 0.f) return;
  float a[3], b[3], n[3], w[3], u[3], vn[3], v[3];
  diffs(cam, dep, ps, W, mx, my, z_depth, a, b);
  cross3(a, b, n);
  world_normal(cam, normals + 3 * mi, world, w);
#pragma unroll
  for (int k = 0; k < 3; ++k) u[k] = sc * am * w[k];  // dL/dn_d(m)
  const float l = sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]);
  if (l > 1e-12f) {  // n / |n|
    const float il = 1.f / l;
    const float h[3] = {n[0] * il, n[1] * il, n[2] * il};
    const float hu = h[0] * u[0] + h[1] * u[1] + h[2] * u[2];
#pragma unroll
    for (int k = 0; k < 3; ++k) vn[k] = (u[k] - h[k] * hu) * il;
  } else {  // n / 1e-12 (the floor)
#pragma unroll
    for (int k = 0; k < 3; ++k) vn[k] = u[k] * 1e12f;
  }
  if (which == 0)
    cross3(b, vn, v);  // d(a x b).vn / da
  else
    cross3(vn, a, v);  // d(a x b).vn / db
#pragma unroll
  for (int k = 0; k < 3; ++k) vp[k] += sign * v[k];
}

__global__ void __launch_bounds__(256)
bwd_kernel(int C, int H, int W, const float *__restrict__ normals,
           const float *__restrict__ depths, int64_t ps, const float *__restrict__ alphas,
           const float *__restrict__ camtoworlds, const float *__restrict__ Ks, int z_depth,
           int world, float nl_over_p, float dl_over_p, const float *__restrict__ g_loss,
           float *__restrict__ v_normals, float *__restrict__ v_depths, int64_t vps,
           int zero_rest, float *__restrict__ v_distort) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t HW = (int64_t)H * W;
  if (i >= C * HW) return;
  const float g = g_loss[0];
  if (v_distort) v_distort[i] = g * dl_over_p;
  if (!v_normals) return;
  const int c = (int)(i / HW);
  const int64_t r = i - c * HW;
  const int y = (int)(r / W), x = (int)(r - (int64_t)y * W);
  const Cam m = load_cam(camtoworlds + 16 * c, Ks + 9 * c);
  const float *dep = depths + c * HW * ps;
  const float *nrm = normals + 3 * c * HW, *alp = alphas + c * HW;
  const float sc = -g * nl_over_p;
  // v_normals = sc * alpha * R^T n_d (world normals: sc * alpha * n_d)
  float vn[3] = {0.f, 0.f, 0.f};
  if (x > 0 && y > 0 && x < W - 1 && y < H - 1) {
    float a[3], b[3], n[3];
    diffs(m, dep, ps, W, x, y, z_depth, a, b);
    cross3(a, b, n);
    const float l = fmaxf(sqrtf(n[0] * n[0] + n[1] * n[1] + n[2] * n[2]), 1e-12f);
    const float s = sc * alp[r] / l;
    if (world) {
#pragma unroll
      for (int k = 0; k < 3; ++k) vn[k] = s * n[k];
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) vn[k] = s * (m.R[k] * n[0] + m.R[3 + k] * n[1] + m.R[6 + k] * n[2]);
    }
  }
  v_normals[3 * i] = vn[0];
  v_normals[3 * i + 1] = vn[1];
  v_normals[3 * i + 2] = vn[2];
  // v_depth: q is the lower point of (x, y-1)'s a, the upper of (x, y+1)'s,
  // the right point of (x-1, y)'s b, the left of (x+1, y)'s
  float vp[3] = {0.f, 0.f, 0.f};
  neighbour_vjp(m, dep, ps, nrm, alp, H, W, x, y - 1, z_depth, world, sc, 0, 1.f, vp);
  neighbour_vjp(m, dep, ps, nrm, alp, H, W, x, y + 1, z_depth, world, sc, 0, -1.f, vp);
  neighbour_vjp(m, dep, ps, nrm, alp, H, W, x - 1, y, z_depth, world, sc, 1, 1.f, vp);
  neighbour_vjp(m, dep, ps, nrm, alp, H, W, x + 1, y, z_depth, world, sc, 1, -1.f, vp);
  float d[3];
  ray_dir(m, x, y, z_depth, d);
  float *vd = v_depths + i * vps;
  if (zero_rest)  // v_depths is the last channel of a [C,H,W,vps] gradient: zero the others
    for (int64_t k = 1; k < vps; ++k) vd[-k] = 0.f;
  vd[0] = d[0] * vp[0] + d[1] * vp[1] + d[2] * vp[2];
}

}  // namespace geomk
}  // namespace gs

using namespace gs;

static inline int64_t geom_loss_blocks(int C, int H, int W) {
  return ((int64_t)C * H * W + 255) / 256;
}

extern "C" int64_t gsplat_hip_geom_loss_2dgs_workspace_bytes(int C, int H, int W) {
  if (C < 0 || H < 0 || W < 0) return 0;
  return geom_loss_blocks(C, H, W) * 2 * (int64_t)sizeof(float);
}

extern "C" int gsplat_hip_geom_loss_2dgs_fwd(int C, int H, int W, const float *normals,
                                             const float *depths, int64_t depth_stride,
                                             const float *alphas, const float *distort,
                                             const float *camtoworlds, const float *Ks,
                                             int z_depth, int world_normals,
                                             float normal_lambda, float dist_lambda, float *out,
                                             void *workspace, void *stream) {
  GS_REQUIRE(C >= 1 && H >= 1 && W >= 1, "geom_loss_2dgs_fwd: empty image");
  const int64_t blocks = geom_loss_blocks(C, H, W);
  GS_REQUIRE(blocks <= 0x7fffffff, "geom_loss_2dgs_fwd: too many pixels");
  const int do_n = normal_lambda != 0.f, do_d = dist_lambda != 0.f;
  GS_REQUIRE(out && workspace, "geom_loss_2dgs_fwd: null out / workspace");
  GS_REQUIRE(((uintptr_t)workspace & 7) == 0, "geom_loss_2dgs_fwd: workspace must be 8-B aligned");
  GS_REQUIRE(!do_n || (normals && depths && alphas && camtoworlds && Ks),
             "geom_loss_2dgs_fwd: null pointer (normal term)");
  GS_REQUIRE(!do_n || depth_stride >= 1, "geom_loss_2dgs_fwd: depth_stride %lld < 1",
             (long long)depth_stride);
  GS_REQUIRE(!do_d || distort, "geom_loss_2dgs_fwd: null distort");
  float *partials = reinterpret_cast<float *>(workspace);
  hipLaunchKernelGGL(geomk::fwd_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, C, H, W, normals, depths, depth_stride, alphas, distort,
                     camtoworlds, Ks, z_depth, world_normals, do_n, do_d, partials);
  GS_CHECK_LAUNCH("geom_loss_2dgs_fwd");
  hipLaunchKernelGGL(geomk::finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, blocks,
                     partials, 1.0 / ((double)C * H * W), normal_lambda, dist_lambda, out);
  GS_CHECK_LAUNCH("geom_loss_2dgs_fwd (finish)");
  return 0;
}

extern "C" int gsplat_hip_geom_loss_2dgs_bwd(int C, int H, int W, const float *normals,
                                             const float *depths, int64_t depth_stride,
                                             const float *alphas, const float *camtoworlds,
                                             const float *Ks, int z_depth, int world_normals,
                                             float normal_lambda, float dist_lambda,
                                             const float *g_loss, float *v_normals,
                                             float *v_depths, int64_t v_depth_stride,
                                             int zero_rest, float *v_distort, void *stream) {
  GS_REQUIRE(C >= 1 && H >= 1 && W >= 1, "geom_loss_2dgs_bwd: empty image");
  const int64_t blocks = geom_loss_blocks(C, H, W);
  GS_REQUIRE(blocks <= 0x7fffffff, "geom_loss_2dgs_bwd: too many pixels");
  const int do_n = normal_lambda != 0.f, do_d = dist_lambda != 0.f;
  GS_REQUIRE(g_loss, "geom_loss_2dgs_bwd: null g_loss");
  GS_REQUIRE(!do_n || (normals && depths && alphas && camtoworlds && Ks && v_normals && v_depths),
             "geom_loss_2dgs_bwd: null pointer (normal term)");
  GS_REQUIRE(!do_n || (depth_stride >= 1 && v_depth_stride >= 1),
             "geom_loss_2dgs_bwd: depth strides %lld, %lld < 1", (long long)depth_stride,
             (long long)v_depth_stride);
  GS_REQUIRE(!do_d || v_distort, "geom_loss_2dgs_bwd: null v_distort");
  if (!do_n && !do_d) return 0;
  const double inv_p = 1.0 / ((double)C * H * W);
  hipLaunchKernelGGL(geomk::bwd_kernel, dim3((unsigned)blocks), dim3(256), 0,
                     (hipStream_t)stream, C, H, W, normals, depths, depth_stride, alphas,
                     camtoworlds, Ks, z_depth, world_normals, (float)(normal_lambda * inv_p),
                     (float)(dist_lambda * inv_p), g_loss, do_n ? v_normals : nullptr,
                     do_n ? v_depths : nullptr, v_depth_stride, zero_rest,
                     do_d ? v_distort : nullptr);
  GS_CHECK_LAUNCH("geom_loss_2dgs_bwd");
  return 0;
}
