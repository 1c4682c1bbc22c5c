// Sparse depth supervision of the 3DGS trainer (simple_trainer.py depth_loss,
// :647-665), fused: for the M points (x, y, d_gt) of one image
//
//   ed   = sum_k w_k D_k / max(alpha_k, 1e-10)     (bilinear, zero padding)
//   disp = ed > 0 ? 1 / ed : 0
//   L    = mean_j |disp_j - 1 / d_gt_j|            (0 for M = 0)
//
// The reference divides the whole depth image by alpha (RGB+ED), slices and
// permutes it and runs grid_sample(align_corners=True) at the points: with
// align_corners the normalise / un-normalise round trip is the identity, so
// the sample position is (x, y) in pixels, the corners floor and floor + 1
// with grid_sample's own weights, and only the 4 M corner pixels are read.
// The division happens at the corners, before the interpolation, as in the
// reference.
//
// The points of all images live in CSR tables on the device (points[sum M, 3],
// offsets i32[n_images + 1]); the image is chosen by a device int64, so one
// kernel node of a captured step serves every image: the grid is sized for
// the table's largest M, workgroups past the image's count exit at once.
//
// Forward: one launch.  A lane per point; wave butterfly, the workgroup's four
// waves in index order, one partial per workgroup; the workgroup that takes
// the last ticket adds the partials in index order (double) and writes the
// mean -- bit-identical between calls, no pre-zeroed accumulator (the ticket
// is left at 0 again).  It also stores each point's unit gradient dL/d ed.
// Backward: the scatter to D_k and alpha_k of the four corners with float
// atomics (points share pixels), after a zero fill by kernel of the planes
// that receive it.
#include "wave_ops.h"

namespace gs {
namespace depthk {

constexpr float kAlphaFloor = 1e-10f;

struct Table {
  const float *points;      // [sum M, 3]: x, y, d_gt
  const int32_t *offsets;   // [n_images + 1]
  const int64_t *cam_index; // [1]
  int n_images;
  int max_points;         // rows of `unit`: an image's count is clamped to it
};

// (first row, count) of the chosen image; the index is clamped to the table
GS_INLINE void image_rows(const Table &t, int &first, int &count) {
  int64_t i = t.cam_index[0];
  i = i < 0 ? 0 : (i >= t.n_images ? t.n_images - 1 : i);
  first = t.offsets[i];
  count = t.offsets[i + 1] - first;
  count = count < 0 ? 0 : (count > t.max_points ? t.max_points : count);
}

struct Corners {
  int64_t pix[4];  // pixel index y * W + x, -1: outside (zero padding)
  float w[4];      // grid_sample's order: nw, ne, sw, se
};

GS_INLINE Corners corners_of(float x, float y, int H, int W) {
  Corners c;
  const float x0 = floorf(x), y0 = floorf(y);
  // a position whose cell lies wholly outside (or NaN): no corner is read
  const bool any = x0 >= -1.f && x0 < (float)W && y0 >= -1.f && y0 < (float)H;
  const int xi = any ? (int)x0 : -2, yi = any ? (int)y0 : -2;
  const float wx1 = x - x0, wx0 = (x0 + 1.f) - x;
  const float wy1 = y - y0, wy0 = (y0 + 1.f) - y;
  c.w[0] = wx0 * wy0, c.w[1] = wx1 * wy0, c.w[2] = wx0 * wy1, c.w[3] = wx1 * wy1;
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int cx = xi + (k & 1), cy = yi + (k >> 1);
    const bool in = any && cx >= 0 && cx < W && cy >= 0 && cy < H;
    c.pix[k] = in ? (int64_t)cy * W + cx : -1;
  }
  return c;
}

__global__ void __launch_bounds__(256)
fwd_kernel(int H, int W, const float *__restrict__ depths, int64_t ds,
           const float *__restrict__ alphas, int64_t as, Table t, float *__restrict__ out,
           float *__restrict__ unit, int32_t *__restrict__ ticket, float *__restrict__ partials) {
  int first, M;
  image_rows(t, first, M);
  const int nb = M > 0 ? (M + 255) / 256 : 1;  // the workgroups with work
  if ((int)blockIdx.x >= nb) return;
  const int j = blockIdx.x * 256 + threadIdx.x;
  float term = 0.f;
  if (j < M) {
    const float *p = t.points + 3 * (int64_t)(first + j);
    const float dgt = p[2];
    const Corners c = corners_of(p[0], p[1], H, W);
    float ed = 0.f;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      if (c.pix[k] < 0) continue;
      const float a = alphas ? fmaxf(alphas[c.pix[k] * as], kAlphaFloor) : 1.f;
      ed += c.w[k] * (depths[c.pix[k] * ds] / a);
    }
    const float disp = ed > 0.f ? 1.f / ed : 0.f;
    const float diff = disp - 1.f / dgt;
    term = fabsf(diff);
    const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
    unit[j] = ed > 0.f ? sgn * (-1.f / (ed * ed)) / (float)M : 0.f;
  }
  term = wave_sum(term);
  __shared__ float s[4];
  __shared__ int s_last;
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = term;
  __syncthreads();
  if (threadIdx.x == 0) {
    __hip_atomic_store(partials + blockIdx.x, ((s[0] + s[1]) + s[2]) + s[3], __ATOMIC_RELAXED,
                       __HIP_MEMORY_SCOPE_AGENT);
    s_last = __hip_atomic_fetch_add(ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT) ==
             nb - 1;
  }
  __syncthreads();
  if (!s_last) return;
  // the last workgroup to finish: lane t adds partials t, t + 256, ... in order
  double sum = 0.0;
  for (int k = threadIdx.x; k < nb; k += 256)
    sum += (double)__hip_atomic_load(partials + k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) sum += __shfl_xor(sum, m, kWave);
  __shared__ double sd[4];
  if ((threadIdx.x & 63) == 0) sd[threadIdx.x >> 6] = sum;
  __syncthreads();
  if (threadIdx.x == 0) {
    sum = ((sd[0] + sd[1]) + sd[2]) + sd[3];
    out[0] = M > 0 ? (float)(sum / (double)M) : 0.f;
    __hip_atomic_store(ticket, 0, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
}

__global__ void __launch_bounds__(256)
bwd_kernel(int H, int W, const float *__restrict__ depths, int64_t ds,
           const float *__restrict__ alphas, int64_t as, Table t,
           const float *__restrict__ unit, const float *__restrict__ g_loss,
           float *__restrict__ v_depths, int64_t vds, float *__restrict__ v_alphas) {
  int first, M;
  image_rows(t, first, M);
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= M) return;
  const float de = g_loss[0] * unit[j];
  if (de == 0.f) return;
  const float *p = t.points + 3 * (int64_t)(first + j);
  const Corners c = corners_of(p[0], p[1], H, W);
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    if (c.pix[k] < 0) continue;
    const float g = c.w[k] * de;
    if (!alphas) {
      atomic_add_f32(v_depths + c.pix[k] * vds, g);
      continue;
    }
    const float a = alphas[c.pix[k] * as];
    atomic_add_f32(v_depths + c.pix[k] * vds, g / fmaxf(a, kAlphaFloor));
    if (a > kAlphaFloor) atomic_add_f32(v_alphas + c.pix[k], -g * depths[c.pix[k] * ds] / (a * a));
  }
}

}  // namespace depthk
}  // namespace gs

using namespace gs;

static inline int64_t depth_loss_blocks(int64_t max_points) {
  return std::max<int64_t>((max_points + 255) / 256, 1);
}

extern "C" int64_t gsplat_hip_depth_loss_workspace_bytes(int64_t max_points) {
  if (max_points < 0) return 0;
  return 16 + depth_loss_blocks(max_points) * (int64_t)sizeof(float);
}

extern "C" int gsplat_hip_depth_loss_fwd(int H, int W, const float *depths, int64_t depth_stride,
                                         const float *alphas, int64_t alpha_stride,
                                         const float *points, const int32_t *offsets,
                                         int n_images, int64_t max_points,
                                         const int64_t *cam_index, float *out, float *unit,
                                         void *workspace, void *stream) {
  GS_REQUIRE(H >= 1 && W >= 1, "depth_loss_fwd: empty image");
  GS_REQUIRE(n_images >= 1 && max_points >= 0 && max_points < (1 << 30),
             "depth_loss_fwd: n_images %d, max_points %lld", n_images, (long long)max_points);
  GS_REQUIRE(depths && offsets && cam_index && out && workspace,
             "depth_loss_fwd: null pointer");
  GS_REQUIRE(max_points == 0 || (points && unit), "depth_loss_fwd: null points / unit");
  GS_REQUIRE(depth_stride >= 1 && (!alphas || alpha_stride >= 1),
             "depth_loss_fwd: strides %lld, %lld < 1", (long long)depth_stride,
             (long long)alpha_stride);
  GS_REQUIRE(((uintptr_t)workspace & 15) == 0, "depth_loss_fwd: workspace must be 16-B aligned");
  const depthk::Table t{points, offsets, cam_index, n_images, (int)max_points};
  int32_t *ticket = reinterpret_cast<int32_t *>(workspace);
  float *partials = reinterpret_cast<float *>(reinterpret_cast<char *>(workspace) + 16);
  hipLaunchKernelGGL(depthk::fwd_kernel, dim3((unsigned)depth_loss_blocks(max_points)), dim3(256),
                     0, (hipStream_t)stream, H, W, depths, depth_stride, alphas, alpha_stride, t,
                     out, unit, ticket, partials);
  GS_CHECK_LAUNCH("depth_loss_fwd");
  return 0;
}

extern "C" int gsplat_hip_depth_loss_bwd(int H, int W, const float *depths, int64_t depth_stride,
                                         const float *alphas, int64_t alpha_stride,
                                         const float *points, const int32_t *offsets,
                                         int n_images, int64_t max_points,
                                         const int64_t *cam_index, const float *unit,
                                         const float *g_loss, float *v_image,
                                         int64_t v_image_stride, int channel, int zero_image,
                                         float *v_alphas, void *stream) {
  GS_REQUIRE(H >= 1 && W >= 1, "depth_loss_bwd: empty image");
  GS_REQUIRE(n_images >= 1 && max_points >= 0 && max_points < (1 << 30),
             "depth_loss_bwd: n_images %d, max_points %lld", n_images, (long long)max_points);
  GS_REQUIRE(depths && offsets && cam_index && g_loss && v_image, "depth_loss_bwd: null pointer");
  GS_REQUIRE(max_points == 0 || (points && unit), "depth_loss_bwd: null points / unit");
  GS_REQUIRE(!alphas || v_alphas, "depth_loss_bwd: alphas without v_alphas");
  GS_REQUIRE(depth_stride >= 1 && (!alphas || alpha_stride >= 1) && v_image_stride >= 1 &&
                 channel >= 0 && channel < v_image_stride,
             "depth_loss_bwd: strides %lld, %lld, %lld, channel %d", (long long)depth_stride,
             (long long)alpha_stride, (long long)v_image_stride, channel);
  hipStream_t st = (hipStream_t)stream;
  const size_t plane = (size_t)H * W * sizeof(float);
  if (zero_image) GS_HIP(zero_async(v_image, plane * (size_t)v_image_stride, st));
  if (alphas) GS_HIP(zero_async(v_alphas, plane, st));
  if (max_points == 0) return 0;
  const depthk::Table t{points, offsets, cam_index, n_images, (int)max_points};
  hipLaunchKernelGGL(depthk::bwd_kernel, dim3((unsigned)depth_loss_blocks(max_points)), dim3(256),
                     0, st, H, W, depths, depth_stride, alphas, alpha_stride, t, unit, g_loss,
                     v_image + channel, v_image_stride, alphas ? v_alphas : nullptr);
  GS_CHECK_LAUNCH("depth_loss_bwd");
  return 0;
}
