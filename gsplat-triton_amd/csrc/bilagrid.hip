// Bilateral-grid colour correction (examples/lib_bilagrid.py: BilateralGrid,
// slice, total_variation_loss), fused.  grids[N,12,L,Hg,Wg] holds one 3-D grid
// of 3x4 affine colour transforms per training image (channel c = 4 i + j is
// element (i, j)).  For pixel (x, y) of image b, with g = grids[grid_index[b]]:
//
//   fx = (x + 0.5) / W * (Wg - 1),  fy = (y + 0.5) / H * (Hg - 1)
//   gray = 0.299 r + 0.587 g + 0.114 b,  fz = clamp(gray, 0, 1) * (L - 1)
//   A[12] = trilinear interpolation of g at (fz, fy, fx)
//   out_i = A[4i] r + A[4i+1] g + A[4i+2] b + A[4i+3]
//
// which is F.grid_sample(mode="bilinear", align_corners=True,
// padding_mode="border") followed by the matmul, without the [H,W,2] pixel
// grid and the [H,W,3,4] matrices ever existing.
//
// Tiling.  A workgroup owns a tw x th pixel tile (64 x 32 unless the host
// shrinks it).  The xy nodes the tile touches form a rectangle of at most
// nxc x nyc nodes (3 x 3 while the tile is no larger than the node spacing);
// their L x 12 coefficients are staged in LDS channel-last, so a pixel's
// eight corners are eight runs of 12 consecutive floats instead of 96 dwords
// scattered over the [12,L,Hg,Wg] layout.  The host shrinks the tile until
// the rectangle fits the LDS budget (an image smaller than the grid, a deep
// grid), down to one pixel (2 x 2 nodes): every shape runs the same kernels.
//
// Backward.  v_rgb is written once per pixel by a kernel tiled like the
// forward.  The grid gradient is a second kernel organised by cell (the pixels
// between four xy nodes): threads keep the weighted sums of a cell chunk's
// pixels in registers, the workgroup adds its lanes' sums in lane order and
// stores one partial slab, and a finish kernel adds the slabs of a node in a
// fixed order INTO v_grids: the caller initialises v_grids (the
// total-variation backward writes every element once; zeros otherwise), so no
// memset is needed.  No atomics anywhere (LDS float atomics measured ~200
// cycles per wave instruction with the lanes of a wave on few addresses: 1.06
// ms for the 1080p backward); v_grids is bit-reproducible.
//
// Total variation: tv = (1/N) sum_d sum (x[i+1] - x[i])^2 / count_d over the
// three grid axes, partial sums per workgroup and one finishing workgroup in
// a fixed order (double), as geom_loss.hip; the backward writes every element
// of v_grids exactly once.
#include "common.h"

namespace gs {
namespace bilak {

constexpr int kThreads = 256;
constexpr int kLdsFloats = 6144;  // per rectangle (24 KB; the backward holds two)

struct Tiling {
  int tw, th;    // pixel tile
  int nxc, nyc;  // node rectangle capacity
  int tx, ty;    // tiles per image
};

// the most nodes a run of `t` pixels can touch along an axis of `n` pixels
// and `g` nodes: the positions span d = (t - 1) (g - 1) / n, floor(f + d) -
// floor(f) <= ceil(d), plus the upper neighbour and one end node.  The 1e-3
// absorbs the float rounding of the device's coordinates.
static inline int node_cap(int t, int n, int g) {
  if (t == 1) return 2;  // one pixel: its two nodes
  const double d = (double)(t - 1) * (double)(g - 1) / (double)n;
  const int64_t c = (int64_t)ceil(d + 1e-3) + 2;
  return (int)std::min<int64_t>(c, g);
}

static inline bool make_tiling(int H, int W, int L, int Hg, int Wg, Tiling *t) {
  int tw = std::min(64, W), th = std::min(32, H);
  for (;;) {
    const int nxc = node_cap(tw, W, Wg), nyc = node_cap(th, H, Hg);
    if ((int64_t)nxc * nyc * L * 12 <= kLdsFloats) {
      t->tw = tw, t->th = th, t->nxc = nxc, t->nyc = nyc;
      t->tx = (W + tw - 1) / tw, t->ty = (H + th - 1) / th;
      return true;
    }
    if (tw == 1 && th == 1) return false;
    if ((nxc >= nyc && tw > 1) || th == 1)
      tw = (tw + 1) / 2;
    else
      th = (th + 1) / 2;
  }
}

// grid coordinate of pixel p along an axis of n pixels and g nodes; monotone
// in p (every operation is), strictly inside [0, g - 1]
GS_INLINE float coord(int p, int n, int g) { return ((float)p + 0.5f) / (float)n * (float)(g - 1); }

// lower node of a coordinate
GS_INLINE int node0(float f, int g) { return min(max((int)floorf(f), 0), g - 2); }

// first node and node count of the pixel run [p0, p1] (p1 inclusive), at most cap
GS_INLINE void node_range(int p0, int p1, int n, int g, int cap, int &lo, int &cnt) {
  lo = node0(coord(p0, n, g), g);
  const int hi = node0(coord(p1, n, g), g) + 1;
  cnt = min(hi - lo + 1, cap);
}

struct Tile {
  int x0, y0, x1, y1;  // pixel rectangle (inclusive)
  int ix, iy, nx, ny;  // node rectangle
};

GS_INLINE Tile tile_of(int tile_x, int tile_y, int H, int W, int Hg, int Wg, const Tiling &t) {
  Tile r;
  r.x0 = tile_x * t.tw, r.y0 = tile_y * t.th;
  r.x1 = min(r.x0 + t.tw, W) - 1, r.y1 = min(r.y0 + t.th, H) - 1;
  node_range(r.x0, r.x1, W, Wg, t.nxc, r.ix, r.nx);
  node_range(r.y0, r.y1, H, Hg, t.nyc, r.iy, r.ny);
  return r;
}

// stage the tile's nodes: s[((ly * nxc + lx) * L + z) * 12 + c]
GS_INLINE void stage(const float *__restrict__ g, int L, int Hg, int Wg, const Tiling &t,
                     const Tile &r, float *__restrict__ s) {
  const int per_node = L * 12;
  const int total = r.ny * t.nxc * per_node;
  for (int e = threadIdx.x; e < total; e += kThreads) {
    const int node = e / per_node, k = e - node * per_node;
    const int ly = node / t.nxc, lx = node - ly * t.nxc;
    if (lx >= r.nx) continue;
    const int z = k / 12, c = k - z * 12;
    s[e] = g[(((int64_t)c * L + z) * Hg + (r.iy + ly)) * Wg + (r.ix + lx)];
  }
}

struct Pix {
  int base;        // LDS offset of corner (z0, ly, lx), in floats
  int sx, sy, sz;  // LDS strides to the +x, +y, +z corner
  float wx, wy, wz;
  float gray;
};

GS_INLINE Pix locate(int x, int y, float r, float g, float b, int H, int W, int L, int Hg, int Wg,
                     const Tiling &t, const Tile &tl) {
  Pix p;
  const float fx = coord(x, W, Wg), fy = coord(y, H, Hg);
  const int ix0 = node0(fx, Wg), iy0 = node0(fy, Hg);
  p.wx = fx - (float)ix0, p.wy = fy - (float)iy0;
  p.gray = 0.299f * r + 0.587f * g + 0.114f * b;
  const float fz = fminf(fmaxf(p.gray, 0.f), 1.f) * (float)(L - 1);
  const int z0 = node0(fz, L);
  p.wz = fz - (float)z0;
  // inside the staged rectangle by construction; the clamps keep a rounding
  // surprise inside LDS
  const int lx = min(max(ix0 - tl.ix, 0), t.nxc - 2), ly = min(max(iy0 - tl.iy, 0), t.nyc - 2);
  p.sz = 12, p.sx = L * 12, p.sy = t.nxc * L * 12;
  p.base = (ly * t.nxc + lx) * (L * 12) + z0 * 12;
  return p;
}

GS_INLINE void load12(const float *__restrict__ s, float v[12]) {
  const float4 a = reinterpret_cast<const float4 *>(s)[0];
  const float4 b = reinterpret_cast<const float4 *>(s)[1];
  const float4 c = reinterpret_cast<const float4 *>(s)[2];
  v[0] = a.x, v[1] = a.y, v[2] = a.z, v[3] = a.w;
  v[4] = b.x, v[5] = b.y, v[6] = b.z, v[7] = b.w;
  v[8] = c.x, v[9] = c.y, v[10] = c.z, v[11] = c.w;
}

// A0 / A1: the bilinear (xy) interpolation on the z0 / z0 + 1 plane
GS_INLINE void planes(const float *__restrict__ s, const Pix &p, float A0[12], float A1[12]) {
  const float w00 = (1.f - p.wx) * (1.f - p.wy), w10 = p.wx * (1.f - p.wy);
  const float w01 = (1.f - p.wx) * p.wy, w11 = p.wx * p.wy;
  float v[12];
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    float *A = k ? A1 : A0;
    const float *q = s + p.base + k * p.sz;
    load12(q, v);
#pragma unroll
    for (int c = 0; c < 12; ++c) A[c] = w00 * v[c];
    load12(q + p.sx, v);
#pragma unroll
    for (int c = 0; c < 12; ++c) A[c] += w10 * v[c];
    load12(q + p.sy, v);
#pragma unroll
    for (int c = 0; c < 12; ++c) A[c] += w01 * v[c];
    load12(q + p.sy + p.sx, v);
#pragma unroll
    for (int c = 0; c < 12; ++c) A[c] += w11 * v[c];
  }
}

__global__ void __launch_bounds__(kThreads)
slice_fwd_kernel(int H, int W, int L, int Hg, int Wg, Tiling t, const float *__restrict__ grids,
                 const int64_t *__restrict__ grid_index, int n_grids,
                 const float *__restrict__ rgb, float *__restrict__ out) {
  extern __shared__ float4 lds4[];
  float *sA = reinterpret_cast<float *>(lds4);
  const int b = blockIdx.z;
  const Tile tl = tile_of(blockIdx.x, blockIdx.y, H, W, Hg, Wg, t);
  const int64_t n = min(max(grid_index[b], (int64_t)0), (int64_t)n_grids - 1);
  stage(grids + n * 12 * L * Hg * Wg, L, Hg, Wg, t, tl, sA);
  __syncthreads();
  const int w = tl.x1 - tl.x0 + 1, cnt = w * (tl.y1 - tl.y0 + 1);
  for (int q = threadIdx.x; q < cnt; q += kThreads) {
    const int dy = q / w, x = tl.x0 + (q - dy * w), y = tl.y0 + dy;
    const int64_t i = (((int64_t)b * H + y) * W + x) * 3;
    const float r = rgb[i], g = rgb[i + 1], bl = rgb[i + 2];
    const Pix p = locate(x, y, r, g, bl, H, W, L, Hg, Wg, t, tl);
    float A0[12], A1[12];
    planes(sA, p, A0, A1);
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      float a[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) a[j] = A0[4 * k + j] + p.wz * (A1[4 * k + j] - A0[4 * k + j]);
      out[i + k] = a[0] * r + a[1] * g + a[2] * bl + a[3];
    }
  }
}

// v_rgb alone: the forward's tiling, every pixel written once
__global__ void __launch_bounds__(kThreads)
slice_bwd_rgb_kernel(int H, int W, int L, int Hg, int Wg, Tiling t,
                     const float *__restrict__ grids, const int64_t *__restrict__ grid_index,
                     int n_grids, const float *__restrict__ rgb, const float *__restrict__ v_out,
                     float *__restrict__ v_rgb) {
  extern __shared__ float4 lds4[];
  float *sA = reinterpret_cast<float *>(lds4);
  const int b = blockIdx.z;
  const Tile tl = tile_of(blockIdx.x, blockIdx.y, H, W, Hg, Wg, t);
  const int64_t n = min(max(grid_index[b], (int64_t)0), (int64_t)n_grids - 1);
  stage(grids + n * 12 * L * Hg * Wg, L, Hg, Wg, t, tl, sA);
  __syncthreads();
  const int w = tl.x1 - tl.x0 + 1, cnt = w * (tl.y1 - tl.y0 + 1);
  for (int q = threadIdx.x; q < cnt; q += kThreads) {
    const int dy = q / w, x = tl.x0 + (q - dy * w), y = tl.y0 + dy;
    const int64_t i = (((int64_t)b * H + y) * W + x) * 3;
    const float c3[3] = {rgb[i], rgb[i + 1], rgb[i + 2]};
    const float vo[3] = {v_out[i], v_out[i + 1], v_out[i + 2]};
    const Pix p = locate(x, y, c3[0], c3[1], c3[2], H, W, L, Hg, Wg, t, tl);
    float A0[12], A1[12];
    planes(sA, p, A0, A1);
    // through the matrix, and through the guidance (dA/dfz = A1 - A0, v_A[4k+j]
    // = v_out_k rgb_j, v_A[4k+3] = v_out_k) while 0 < gray < 1: torch's clamp
    // passes no gradient at or beyond its borders
    float vr[3] = {0.f, 0.f, 0.f}, vz = 0.f;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
#pragma unroll
      for (int j = 0; j < 3; ++j) {
        const float d = A1[4 * k + j] - A0[4 * k + j];
        vz += vo[k] * c3[j] * d;
        vr[j] += (A0[4 * k + j] + p.wz * d) * vo[k];
      }
      vz += vo[k] * (A1[4 * k + 3] - A0[4 * k + 3]);
    }
    if (p.gray > 0.f && p.gray < 1.f) {
      vz *= (float)(L - 1);
      vr[0] += 0.299f * vz, vr[1] += 0.587f * vz, vr[2] += 0.114f * vz;
    }
    v_rgb[i] = vr[0], v_rgb[i + 1] = vr[1], v_rgb[i + 2] = vr[2];
  }
}

// ------------------------------------------------------------ grid gradient
// A cell is the pixel rectangle between four xy nodes: its pixels all update
// those four nodes' columns.  A workgroup owns one cell's rows of one chunk
// (the host splits a cell's rows into `chunks` so that there are enough
// workgroups).  Thread (lane = t / 12, c = t % 12) walks the pixels lane,
// lane + kLanes, ... of the chunk for channel c and keeps the weighted sums of
// kZ guidance levels x 4 corners in registers (a level the pixel does not
// touch gets weight 0: no indexed registers, no atomics); deeper grids take
// ceil(L / kZ) passes.  The lanes' sums go through LDS and are added in lane
// order, so a workgroup's slab [4 corners][L][12] is bit-reproducible.
constexpr int kLanes = 21;  // pixel lanes of a workgroup (21 * 12 = 252 threads)
constexpr int kZ = 8;       // guidance levels per pass

// first pixel of an axis of n pixels and g nodes whose lower node is >= i
GS_INLINE int first_pixel(int i, int n, int g) {
  if (i <= 0) return 0;
  if (i >= g - 1) return n;
  int p = (int)ceilf((float)i * (float)n / (float)(g - 1) - 0.5f);
  p = min(max(p, 0), n);
  while (p > 0 && node0(coord(p - 1, n, g), g) >= i) --p;
  while (p < n && node0(coord(p, n, g), g) < i) ++p;
  return p;
}

__global__ void __launch_bounds__(kThreads)
slice_bwd_grid_kernel(int H, int W, int L, int Hg, int Wg, int chunks,
                      const float *__restrict__ rgb, const float *__restrict__ v_out,
                      float *__restrict__ slabs) {
  __shared__ float red[kLanes][kZ * 4 * 12];
  const int cell = blockIdx.x, chunk = blockIdx.y, b = blockIdx.z;
  const int cy = cell / (Wg - 1), cx = cell - cy * (Wg - 1);
  const int x0 = first_pixel(cx, W, Wg), x1 = first_pixel(cx + 1, W, Wg);
  const int ya = first_pixel(cy, H, Hg), yb = first_pixel(cy + 1, H, Hg);
  const int y0 = ya + (int)((int64_t)(yb - ya) * chunk / chunks);
  const int y1 = ya + (int)((int64_t)(yb - ya) * (chunk + 1) / chunks);
  const int w = x1 - x0, cnt = w * (y1 - y0);
  const int lane = threadIdx.x / 12, c = threadIdx.x - lane * 12;
  const int ci = c >> 2, cj = c & 3;
  float *dst = slabs + (((int64_t)b * gridDim.y + chunk) * gridDim.x + cell) * (4 * L * 12);
  for (int zb = 0; zb < L; zb += kZ) {
    float acc[kZ][4];
#pragma unroll
    for (int z = 0; z < kZ; ++z) acc[z][0] = acc[z][1] = acc[z][2] = acc[z][3] = 0.f;
    if (lane < kLanes) {
      for (int q = lane; q < cnt; q += kLanes) {
        const int dy = q / w, x = x0 + (q - dy * w), y = y0 + dy;
        const int64_t i = (((int64_t)b * H + y) * W + x) * 3;
        const float r = rgb[i], g = rgb[i + 1], bl = rgb[i + 2];
        const float wx = coord(x, W, Wg) - (float)cx, wy = coord(y, H, Hg) - (float)cy;
        const float gray = 0.299f * r + 0.587f * g + 0.114f * bl;
        const float fz = fminf(fmaxf(gray, 0.f), 1.f) * (float)(L - 1);
        const int z0 = node0(fz, L);
        const float wz = fz - (float)z0;
        // v_A[4i+j] = v_out_i rgb_j, v_A[4i+3] = v_out_i
        const float va = v_out[i + ci] * (cj == 0 ? r : cj == 1 ? g : cj == 2 ? bl : 1.f);
        const float w00 = (1.f - wx) * (1.f - wy) * va, w10 = wx * (1.f - wy) * va;
        const float w01 = (1.f - wx) * wy * va, w11 = wx * wy * va;
        const int zr = z0 - zb;
#pragma unroll
        for (int z = 0; z < kZ; ++z) {
          const float cz = zr == z ? 1.f - wz : (zr + 1 == z ? wz : 0.f);
          acc[z][0] += cz * w00, acc[z][1] += cz * w10;
          acc[z][2] += cz * w01, acc[z][3] += cz * w11;
        }
      }
#pragma unroll
      for (int z = 0; z < kZ; ++z)
#pragma unroll
        for (int k = 0; k < 4; ++k) red[lane][(k * kZ + z) * 12 + c] = acc[z][k];
    }
    __syncthreads();
    // the lanes in order; slab element (k, zb + z, c)
    for (int e = threadIdx.x; e < kZ * 4 * 12; e += kThreads) {
      const int k = e / (kZ * 12), z = (e - k * kZ * 12) / 12;
      if (zb + z < L) {
        float sum = 0.f;
        for (int l = 0; l < kLanes; ++l) sum += red[l][e];
        dst[(k * L + zb + z) * 12 + (e % 12)] = sum;
      }
    }
    __syncthreads();
  }
}

// One thread per (node, z, c) of an image's grid.  Image b is handled when
// it is the first of the batch with its grid index; it then also takes the
// later images of that index, so every element of v_grids is updated by one
// thread, in a fixed order: images, the node's up to four cells, chunks.
__global__ void __launch_bounds__(kThreads)
slice_finish_kernel(int B, int L, int Hg, int Wg, int chunks,
                    const int64_t *__restrict__ grid_index, int n_grids,
                    const float *__restrict__ slabs, float *__restrict__ v_grids) {
  const int b = blockIdx.y;
  const int per_node = L * 12;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  if (e >= Hg * Wg * per_node) return;
  const int64_t n = min(max(grid_index[b], (int64_t)0), (int64_t)n_grids - 1);
  for (int o = 0; o < b; ++o)
    if (min(max(grid_index[o], (int64_t)0), (int64_t)n_grids - 1) == n) return;
  const int node = e / per_node, zc = e - node * per_node;
  const int iy = node / Wg, ix = node - iy * Wg;
  const int z = zc / 12, c = zc - z * 12;
  const int cells = (Wg - 1) * (Hg - 1), slab = 4 * per_node;
  float acc = 0.f;
  for (int o = b; o < B; ++o) {
    if (o != b && min(max(grid_index[o], (int64_t)0), (int64_t)n_grids - 1) != n) continue;
    for (int cy = max(iy - 1, 0); cy <= min(iy, Hg - 2); ++cy)
      for (int cx = max(ix - 1, 0); cx <= min(ix, Wg - 2); ++cx) {
        const int k = (ix - cx) + 2 * (iy - cy);  // the node's corner in that cell
        for (int s = 0; s < chunks; ++s)
          acc += slabs[(((int64_t)o * chunks + s) * cells + cy * (Wg - 1) + cx) * slab +
                       k * per_node + zc];
      }
  }
  v_grids[n * 12 * L * Hg * Wg + (((int64_t)c * L + z) * Hg + iy) * Wg + ix] += acc;
}

// ---------------------------------------------------------- total variation
struct TvScale {
  float sl, sy, sx;  // 1 / count_d of the three axes
};

__global__ void __launch_bounds__(kThreads)
tv_fwd_kernel(int per_grid, int L, int Hg, int Wg, TvScale sc, const float *__restrict__ grids,
              float *__restrict__ partials) {
  // blockIdx.y: the grid; i: the element of its [12,L,Hg,Wg] (32-bit index math)
  const int i = blockIdx.x * kThreads + threadIdx.x;
  const float *g = grids + (int64_t)blockIdx.y * per_grid;
  float v = 0.f;
  if (i < per_grid) {
    const int sZ = Wg * Hg;
    const int x = i % Wg, y = (i / Wg) % Hg, z = (i / sZ) % L;
    const float c = g[i];
    if (x + 1 < Wg) {
      const float d = g[i + 1] - c;
      v += sc.sx * d * d;
    }
    if (y + 1 < Hg) {
      const float d = g[i + Wg] - c;
      v += sc.sy * d * d;
    }
    if (z + 1 < L) {
      const float d = g[i + sZ] - c;
      v += sc.sl * d * d;
    }
  }
  v = wave_sum(v);
  __shared__ float s[4];
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0)
    partials[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = ((s[0] + s[1]) + s[2]) + s[3];
}

GS_INLINE double wave_sum_f64(double v) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) v += __shfl_xor(v, m, kWave);
  return v;
}

// one workgroup: lane t sums partials t, t + 256, ... in that order (double),
// then the wave butterfly and the four waves in index order
__global__ void __launch_bounds__(kThreads)
tv_finish_kernel(int64_t n_partials, const float *__restrict__ partials, double inv_n,
                 float scale, float *__restrict__ out) {
  double a = 0.0;
  for (int64_t k = threadIdx.x; k < n_partials; k += kThreads) a += (double)partials[k];
  a = wave_sum_f64(a);
  __shared__ double s[4];
  if ((threadIdx.x & 63) == 0) s[threadIdx.x >> 6] = a;
  __syncthreads();
  if (threadIdx.x == 0) {
    const float tv = (float)((((s[0] + s[1]) + s[2]) + s[3]) * inv_n);
    out[0] = scale * tv;
    out[1] = tv;
  }
}

// v_grids[i] = g_loss * scale * dtv/dx[i]: every element written once
// (two_over_n = 2 scale / N)
__global__ void __launch_bounds__(kThreads)
tv_bwd_kernel(int per_grid, int L, int Hg, int Wg, TvScale sc, float two_over_n,
              const float *__restrict__ grids, const float *__restrict__ g_loss,
              float *__restrict__ v_all) {
  const int i = blockIdx.x * kThreads + threadIdx.x;
  if (i >= per_grid) return;
  const float *g = grids + (int64_t)blockIdx.y * per_grid;
  float *v_grids = v_all + (int64_t)blockIdx.y * per_grid;
  const int sY = Wg, sZ = Wg * Hg;
  const int x = i % Wg, y = (i / Wg) % Hg, z = (i / sZ) % L;
  const float c = g[i];
  float v = 0.f;
  if (x > 0) v += sc.sx * (c - g[i - 1]);
  if (x + 1 < Wg) v -= sc.sx * (g[i + 1] - c);
  if (y > 0) v += sc.sy * (c - g[i - sY]);
  if (y + 1 < Hg) v -= sc.sy * (g[i + sY] - c);
  if (z > 0) v += sc.sl * (c - g[i - sZ]);
  if (z + 1 < L) v -= sc.sl * (g[i + sZ] - c);
  v_grids[i] = g_loss[0] * two_over_n * v;
}

}  // namespace bilak
}  // namespace gs

using namespace gs;

static int bilagrid_check(const char *who, int B, int H, int W, int N, int L, int Hg, int Wg,
                          bilak::Tiling *t) {
  GS_REQUIRE(B >= 1 && H >= 1 && W >= 1 && N >= 1, "%s: empty batch, image or grid set", who);
  GS_REQUIRE(L >= 2 && Hg >= 2 && Wg >= 2, "%s: every grid dimension must be >= 2, got (%d,%d,%d)",
             who, L, Hg, Wg);
  GS_REQUIRE(B <= 65535, "%s: batch %d > 65535", who, B);
  GS_REQUIRE((int64_t)H * W <= 0x3fffffff, "%s: image too large", who);
  GS_REQUIRE((int64_t)12 * L * Hg * Wg <= 0x3fffffff, "%s: grid too large", who);
  GS_REQUIRE(bilak::make_tiling(H, W, L, Hg, Wg, t),
             "%s: guidance dimension %d too deep for the LDS tile (max %d)", who, L,
             bilak::kLdsFloats / 48);
  GS_REQUIRE(t->ty <= 65535, "%s: too many tile rows", who);
  return 0;
}

// chunks of a cell's rows: enough workgroups to fill the device
static inline int grid_chunks(int B, int H, int Hg, int Wg) {
  const int64_t cells = (int64_t)B * (Hg - 1) * (Wg - 1);
  const int64_t want = (1024 + cells - 1) / cells;
  const int64_t rows = std::max<int64_t>(1, H / (Hg - 1));  // pixel rows of a cell
  return (int)std::max<int64_t>(1, std::min<int64_t>(std::min<int64_t>(want, rows), 64));
}

extern "C" int64_t gsplat_hip_bilagrid_slice_workspace_bytes(int B, int H, int W, int L, int Hg,
                                                             int Wg) {
  bilak::Tiling t;
  if (bilagrid_check("bilagrid_slice_workspace_bytes", B, H, W, 1, L, Hg, Wg, &t)) return 0;
  return (int64_t)B * grid_chunks(B, H, Hg, Wg) * (Hg - 1) * (Wg - 1) * 4 * L * 12 *
         (int64_t)sizeof(float);
}

extern "C" int gsplat_hip_bilagrid_slice_fwd(int B, int H, int W, int N, int L, int Hg, int Wg,
                                             const float *grids, const int64_t *grid_index,
                                             const float *rgb, float *out, void *stream) {
  bilak::Tiling t;
  if (int rc = bilagrid_check("bilagrid_slice_fwd", B, H, W, N, L, Hg, Wg, &t)) return rc;
  GS_REQUIRE(grids && grid_index && rgb && out, "bilagrid_slice_fwd: null pointer");
  const size_t lds = (size_t)t.nyc * t.nxc * L * 12 * sizeof(float);
  hipLaunchKernelGGL(bilak::slice_fwd_kernel, dim3(t.tx, t.ty, B), dim3(bilak::kThreads), lds,
                     (hipStream_t)stream, H, W, L, Hg, Wg, t, grids, grid_index, N, rgb, out);
  GS_CHECK_LAUNCH("bilagrid_slice_fwd");
  return 0;
}

extern "C" int gsplat_hip_bilagrid_slice_bwd(int B, int H, int W, int N, int L, int Hg, int Wg,
                                             const float *grids, const int64_t *grid_index,
                                             const float *rgb, const float *v_out, float *v_rgb,
                                             float *v_grids, void *workspace, void *stream) {
  bilak::Tiling t;
  if (int rc = bilagrid_check("bilagrid_slice_bwd", B, H, W, N, L, Hg, Wg, &t)) return rc;
  GS_REQUIRE(grids && grid_index && rgb && v_out && v_rgb && v_grids && workspace,
             "bilagrid_slice_bwd: null pointer");
  GS_REQUIRE(((uintptr_t)workspace & 15) == 0, "bilagrid_slice_bwd: workspace must be 16-B aligned");
  const size_t lds = (size_t)t.nyc * t.nxc * L * 12 * sizeof(float);
  float *slabs = reinterpret_cast<float *>(workspace);
  hipLaunchKernelGGL(bilak::slice_bwd_rgb_kernel, dim3(t.tx, t.ty, B), dim3(bilak::kThreads), lds,
                     (hipStream_t)stream, H, W, L, Hg, Wg, t, grids, grid_index, N, rgb, v_out,
                     v_rgb);
  GS_CHECK_LAUNCH("bilagrid_slice_bwd (rgb)");
  const int chunks = grid_chunks(B, H, Hg, Wg);
  hipLaunchKernelGGL(bilak::slice_bwd_grid_kernel, dim3((Hg - 1) * (Wg - 1), chunks, B),
                     dim3(bilak::kThreads), 0, (hipStream_t)stream, H, W, L, Hg, Wg, chunks, rgb,
                     v_out, slabs);
  GS_CHECK_LAUNCH("bilagrid_slice_bwd (grid)");
  const int per_image = Hg * Wg * L * 12;
  hipLaunchKernelGGL(bilak::slice_finish_kernel,
                     dim3((per_image + bilak::kThreads - 1) / bilak::kThreads, B),
                     dim3(bilak::kThreads), 0, (hipStream_t)stream, B, L, Hg, Wg, chunks,
                     grid_index, N, slabs, v_grids);
  GS_CHECK_LAUNCH("bilagrid_slice_bwd (finish)");
  return 0;
}

static inline bilak::TvScale tv_scale(int L, int Hg, int Wg) {
  bilak::TvScale s;
  s.sl = (float)(1.0 / (12.0 * (L - 1) * Hg * Wg));
  s.sy = (float)(1.0 / (12.0 * L * (Hg - 1) * Wg));
  s.sx = (float)(1.0 / (12.0 * L * Hg * (Wg - 1)));
  return s;
}

// blocks: workgroups per grid (grid.x; grid.y = N)
static int tv_check(const char *who, int N, int L, int Hg, int Wg, int64_t *blocks) {
  GS_REQUIRE(N >= 1 && N <= 65535, "%s: 1 to 65535 grids, got %d", who, N);
  GS_REQUIRE(L >= 2 && Hg >= 2 && Wg >= 2, "%s: every grid dimension must be >= 2, got (%d,%d,%d)",
             who, L, Hg, Wg);
  GS_REQUIRE((int64_t)12 * L * Hg * Wg <= 0x3fffffff, "%s: grid too large", who);
  *blocks = ((int64_t)12 * L * Hg * Wg + bilak::kThreads - 1) / bilak::kThreads;
  return 0;
}

extern "C" int64_t gsplat_hip_bilagrid_tv_workspace_bytes(int N, int L, int Hg, int Wg) {
  int64_t blocks;
  if (tv_check("bilagrid_tv_workspace_bytes", N, L, Hg, Wg, &blocks)) return 0;
  return blocks * N * (int64_t)sizeof(float);
}

extern "C" int gsplat_hip_bilagrid_tv_fwd(int N, int L, int Hg, int Wg, const float *grids,
                                          float scale, float *out, void *workspace,
                                          void *stream) {
  int64_t blocks;
  if (int rc = tv_check("bilagrid_tv_fwd", N, L, Hg, Wg, &blocks)) return rc;
  GS_REQUIRE(grids && out && workspace, "bilagrid_tv_fwd: null pointer");
  float *partials = reinterpret_cast<float *>(workspace);
  hipLaunchKernelGGL(bilak::tv_fwd_kernel, dim3((unsigned)blocks, N), dim3(bilak::kThreads), 0,
                     (hipStream_t)stream, 12 * L * Hg * Wg, L, Hg, Wg, tv_scale(L, Hg, Wg), grids,
                     partials);
  GS_CHECK_LAUNCH("bilagrid_tv_fwd");
  hipLaunchKernelGGL(bilak::tv_finish_kernel, dim3(1), dim3(bilak::kThreads), 0,
                     (hipStream_t)stream, blocks * N, partials, 1.0 / (double)N, scale, out);
  GS_CHECK_LAUNCH("bilagrid_tv_fwd (finish)");
  return 0;
}

extern "C" int gsplat_hip_bilagrid_tv_bwd(int N, int L, int Hg, int Wg, const float *grids,
                                          float scale, const float *g_loss, float *v_grids,
                                          void *stream) {
  int64_t blocks;
  if (int rc = tv_check("bilagrid_tv_bwd", N, L, Hg, Wg, &blocks)) return rc;
  GS_REQUIRE(grids && g_loss && v_grids, "bilagrid_tv_bwd: null pointer");
  hipLaunchKernelGGL(bilak::tv_bwd_kernel, dim3((unsigned)blocks, N), dim3(bilak::kThreads), 0,
                     (hipStream_t)stream, 12 * L * Hg * Wg, L, Hg, Wg, tv_scale(L, Hg, Wg),
                     (float)(2.0 * (double)scale / (double)N), grids, g_loss, v_grids);
  GS_CHECK_LAUNCH("bilagrid_tv_bwd");
  return 0;
}
