// Exact k-nearest neighbours of a static 3-D point cloud (examples/utils.py:141
// knn, the search behind the SfM scale initialisation), for gfx950.
//
// Order: row i holds the k points with the smallest (d2, index), d2 =
// ((dx*dx) + (dy*dy)) + (dz*dz) in float64 on the float32 coordinates with no
// contraction into FMAs, the lower index winning a tie.  The result therefore
// equals a brute-force float64 search index for index, in every run.
//
// Layout: one multi-resolution grid for the price of one sort.
//   box      two-stage min/max of the points (no float atomics) -> Box
//   keys     cell = min(2^20 - 1, floor((x - lo) * inv)) per axis in float64;
//            60-bit Morton key, 20 bits per axis.  The cell of level l (edge
//            2^l finest cells) is cell >> l, its points the keys that share
//            the prefix key >> 3l: one contiguous range of the sorted keys.
//   sort     two stable lsd_sort_pairs runs (low 30 bits, then the high 30
//            bits gathered through the first permutation)
//   gather   sorted 16-B records (x, y, z, original index) and 64-bit keys;
//            separate queries are sorted the same way with the points' box
//   search   one workgroup per 256 consecutive sorted queries, one query per
//            lane, the k best (d2, index) pairs in registers (no scratch).
//
// The search walks the levels upward, all lanes of a workgroup together.  A
// lane starts at the finest level at which its own cell holds k points.  At a
// level it needs the 3x3x3 block of cells around its own.  The workgroup takes
// the union box of its lanes' blocks; with at most CAP cells in it the lanes
// look the cells' ranges up cooperatively (two binary searches per cell,
// once), the ranges are staged through LDS in chunks of CH records and every
// lane scans a chunk by uniform (broadcast) 16-B LDS reads, taking a record
// when its cell lies inside the lane's own block.  A larger union box (Morton
// order jumps at octant boundaries) makes the lanes read their own 27 ranges
// from global memory instead.  Both paths see exactly the points of the block.
//
// A lane is done when its k-th d2 is below the squared distance from the query
// to the nearest face of its block that is not on the border of the grid; the
// face distance is shrunk by a margin that covers the rounding of the cell
// formula (face_bound2).  Otherwise it clears its list and repeats one level
// up; at level 20 the block is the whole grid and the lane finishes, so the
// walk is at most 21 levels whatever the data.
//
// LDS per workgroup: CH = 1024 records (16 KB) and their cell codes (4 KB),
// the CAP = 512 cell ranges (4 KB): 24 KB, six workgroups per CU by LDS, so
// the occupancy is set by the registers of the k-list, not by the staging.
#include <limits.h>

#include "common.h"
#include "lsd_sort.h"
#include "scan_ops.h"
#include "wave_ops.h"

namespace gs {
namespace knn {

constexpr int NT = 256;
constexpr int LV = 20;  // bits per axis = the top level
constexpr int NCELL = 1 << LV;
constexpr int BOX_BLOCKS = 1024;
constexpr int CAP = 2 * NT;  // union-box cells looked up cooperatively (two per lane)
constexpr int CH = 1024;     // records per LDS chunk
constexpr int64_t MAX_POINTS = (int64_t)1 << 30;

// lo, inv = 2^20 / extent (0: no extent, or a non-finite box -> cell 0),
// edge = extent / 2^20, margin: see face_bound2
struct Box {
  double lo[3], inv[3], edge[3], margin[3];
};

GS_INLINE int cell_of(float x, double lo, double inv) {
  const double c = ((double)x - lo) * inv;
  return c >= 0.0 ? (c < (double)NCELL ? (int)c : NCELL - 1) : 0;  // NaN -> 0
}

// bit i of v -> bit 3i (v < 2^21)
GS_INLINE uint64_t spread3(uint32_t v) {
  uint64_t x = v & 0x1fffffu;
  x = (x | x << 32) & 0x1f00000000ffffull;
  x = (x | x << 16) & 0x1f0000ff0000ffull;
  x = (x | x << 8) & 0x100f00f00f00f00full;
  x = (x | x << 4) & 0x10c30c30c30c30c3ull;
  x = (x | x << 2) & 0x1249249249249249ull;
  return x;
}

GS_INLINE uint64_t morton(int cx, int cy, int cz) {
  return spread3((uint32_t)cx) | (spread3((uint32_t)cy) << 1) | (spread3((uint32_t)cz) << 2);
}

GS_INLINE uint64_t key_of(const float *__restrict__ pts, int64_t i, const Box &b) {
  return morton(cell_of(pts[3 * i], b.lo[0], b.inv[0]), cell_of(pts[3 * i + 1], b.lo[1], b.inv[1]),
                cell_of(pts[3 * i + 2], b.lo[2], b.inv[2]));
}

// ------------------------------------------------------------------- box
// fminf / fmaxf drop a NaN operand; an all-NaN or infinite cloud gives a box
// that box_final_kernel maps to inv = 0.
GS_INLINE void wave_minmax(float (&mn)[3], float (&mx)[3]) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = fminf(mn[a], __shfl_xor(mn[a], m, kWave));
      mx[a] = fmaxf(mx[a], __shfl_xor(mx[a], m, kWave));
    }
}

// the workgroup's min/max (valid in thread 0)
GS_INLINE void block_minmax(float (&mn)[3], float (&mx)[3], float (*s)[6]) {
  wave_minmax(mn, mx);
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  if (lane == 0)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      s[wid][a] = mn[a];
      s[wid][3 + a] = mx[a];
    }
  __syncthreads();
  if (threadIdx.x == 0)
    for (int w = 1; w < NT / 64; ++w)
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        mn[a] = fminf(mn[a], s[w][a]);
        mx[a] = fmaxf(mx[a], s[w][3 + a]);
      }
}

__global__ void __launch_bounds__(NT)
box_partial_kernel(const float *__restrict__ pts, int64_t n, float *__restrict__ partial) {
  __shared__ float s[NT / 64][6];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x; i < n; i += (int64_t)gridDim.x * NT)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const float v = pts[3 * i + a];
      mn[a] = fminf(mn[a], v);
      mx[a] = fmaxf(mx[a], v);
    }
  block_minmax(mn, mx, s);
  if (threadIdx.x == 0)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      partial[6 * blockIdx.x + a] = mn[a];
      partial[6 * blockIdx.x + 3 + a] = mx[a];
    }
}

__global__ void __launch_bounds__(NT)
box_final_kernel(const float *__restrict__ partial, int nb, Box *__restrict__ box) {
  __shared__ float s[NT / 64][6];
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int i = threadIdx.x; i < nb; i += NT)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      mn[a] = fminf(mn[a], partial[6 * i + a]);
      mx[a] = fmaxf(mx[a], partial[6 * i + 3 + a]);
    }
  block_minmax(mn, mx, s);
  if (threadIdx.x == 0)
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const double lo = (double)mn[a], ext = (double)mx[a] - lo;
      const bool ok = ext > 0.0 && ext < (double)INFINITY;
      box->lo[a] = lo;
      box->inv[a] = ok ? (double)NCELL / ext : 0.0;
      box->edge[a] = ok ? ext / (double)NCELL : 0.0;
      box->margin[a] = 0x1p-46 * (fabs((double)mn[a]) + fabs((double)mx[a]));
    }
}

// --------------------------------------------------------- keys and gathers
__global__ void __launch_bounds__(NT)
keys_lo_kernel(const float *__restrict__ pts, int64_t n, const Box *__restrict__ box,
               uint32_t *__restrict__ k, int32_t *__restrict__ v) {
  const int64_t i = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (i >= n) return;
  k[i] = (uint32_t)(key_of(pts, i, *box) & 0x3fffffffull);
  v[i] = (int32_t)i;
}

__global__ void __launch_bounds__(NT)
keys_hi_kernel(const float *__restrict__ pts, int64_t n, const Box *__restrict__ box,
               const int32_t *__restrict__ perm, uint32_t *__restrict__ k,
               int32_t *__restrict__ v) {
  const int64_t j = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (j >= n) return;
  const int32_t i = perm[j];
  k[j] = (uint32_t)(key_of(pts, i, *box) >> 30);
  v[j] = i;
}

// keys: null for the queries (the search takes their cells from the records)
__global__ void __launch_bounds__(NT)
gather_kernel(const float *__restrict__ pts, int64_t n, const Box *__restrict__ box,
              const int32_t *__restrict__ perm, float4 *__restrict__ rec,
              uint64_t *__restrict__ keys) {
  const int64_t j = (int64_t)blockIdx.x * NT + threadIdx.x;
  if (j >= n) return;
  const int32_t i = perm[j];
  rec[j] = make_float4(pts[3 * (int64_t)i], pts[3 * (int64_t)i + 1], pts[3 * (int64_t)i + 2],
                       __int_as_float(i));
  if (keys) keys[j] = key_of(pts, i, *box);
}

// ---------------------------------------------------------------- search
GS_INLINE int lower_bound(const uint64_t *__restrict__ keys, int n, uint64_t t) {
  int lo = 0, hi = n;
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    if (keys[mid] < t) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// [s, e): the sorted points in the cell (x, y, z) of level L
GS_INLINE void cell_range(const uint64_t *__restrict__ keys, int n, int x, int y, int z, int L,
                          int &s, int &e) {
  const uint64_t p = morton(x, y, z);
  s = lower_bound(keys, n, p << (3 * L));
  e = lower_bound(keys, n, (p + 1) << (3 * L));
}

GS_INLINE double dist2(double qx, double qy, double qz, const float4 &r) {
#pragma clang fp contract(off)
  const double dx = qx - (double)r.x, dy = qy - (double)r.y, dz = qz - (double)r.z;
  return ((dx * dx) + (dy * dy)) + (dz * dz);
}

GS_INLINE bool before(double d, int i, double e, int j) { return d < e || (d == e && i < j); }

// The k best pairs in ascending order; a candidate that beats the last one
// replaces it and sinks to its place by K - 1 compare-exchanges (all indices
// static: the lists stay in registers).  A NaN d2 never enters.
template <int K>
GS_INLINE void consider(double (&bd)[K], int (&bi)[K], double d, int i) {
  if (!before(d, i, bd[K - 1], bi[K - 1])) return;
  bd[K - 1] = d;
  bi[K - 1] = i;
#pragma unroll
  for (int j = K - 1; j > 0; --j) {
    const bool sw = before(bd[j], bi[j], bd[j - 1], bi[j - 1]);
    const double td = bd[j - 1];
    const int ti = bi[j - 1];
    bd[j - 1] = sw ? bd[j] : td;
    bi[j - 1] = sw ? bi[j] : ti;
    bd[j] = sw ? td : bd[j];
    bi[j] = sw ? ti : bi[j];
  }
}

// Squared distance from the query coordinate q to the faces of its block on
// one axis, below which no point outside the block can lie.  The block covers
// the cells cl - 1 .. cl + 1 of the level (nc cells of edge E on the axis), so
// its faces are the planes lo + (cl - 1) E and lo + (cl + 2) E.  A face on the
// border of the grid (no cell beyond it) does not bound anything.
// Rounding: a point whose cell is i or more satisfies (p - lo) * inv >= i only
// in float64 arithmetic, so it may sit up to ~5 ulp of the extent below the
// plane, and the plane itself carries ~3 ulp of |lo| + extent.  The distance
// is shrunk by margin = 2^-46 (|lo| + |hi|), over 100 ulp of the largest
// coordinate, and by the factor 1 - 2^-40 against the rounding of d2; the
// caller accepts on strict inequality only, so a point at exactly the bound
// with a lower index is never missed.
GS_INLINE double face_bound2(double q, double lo, double E, double margin, int cl, int nc) {
  double b2 = (double)INFINITY;
  if (cl - 1 > 0) {
    const double df = fmax((q - (lo + (double)(cl - 1) * E)) * (1.0 - 0x1p-40) - margin, 0.0);
    b2 = fmin(b2, df * df);
  }
  if (cl + 2 < nc) {
    const double df = fmax(((lo + (double)(cl + 2) * E) - q) * (1.0 - 0x1p-40) - margin, 0.0);
    b2 = fmin(b2, df * df);
  }
  return b2;
}

template <int K>
__global__ void __launch_bounds__(NT)
search_kernel(const float4 *__restrict__ prec, const uint64_t *__restrict__ pkeys, int N,
              const float4 *__restrict__ qrec, int M, int k, const Box *__restrict__ box,
              float *__restrict__ dists, int64_t *__restrict__ idx) {
  __shared__ float4 srec[CH];
  __shared__ uint32_t scode[CH];
  __shared__ int cstart[CAP];
  __shared__ int cpre[CAP + 1];
  __shared__ int sbox[6];
  __shared__ int wsum[NT / 64];
  const int t = threadIdx.x;
  const int64_t g = (int64_t)blockIdx.x * NT + t;
  const bool valid = g < M;
  const float4 q = valid ? qrec[g] : make_float4(0.f, 0.f, 0.f, 0.f);
  const double qd[3] = {(double)q.x, (double)q.y, (double)q.z};
  const Box b = *box;
  const int c[3] = {cell_of(q.x, b.lo[0], b.inv[0]), cell_of(q.y, b.lo[1], b.inv[1]),
                    cell_of(q.z, b.lo[2], b.inv[2])};

  // the finest level at which the lane's own cell holds k points: the count
  // grows with the level and is N >= k at the top
  int start = LV + 1;
  if (valid) {
    int a = 0, z = LV;
    while (a < z) {
      const int m = (a + z) >> 1;
      int s, e;
      cell_range(pkeys, N, c[0] >> m, c[1] >> m, c[2] >> m, m, s, e);
      if (e - s >= k) z = m; else a = m + 1;
    }
    start = a;
  }

  double bd[K];
  int bi[K];
  bool done = !valid;
  for (int L = 0; L <= LV; ++L) {
    const bool act = !done && start <= L;
    const int nc = 1 << (LV - L);
    int lo3[3], hi3[3];
#pragma unroll
    for (int a = 0; a < 3; ++a) {
      const int cl = c[a] >> L;
      lo3[a] = max(cl - 1, 0);
      hi3[a] = min(cl + 1, nc - 1);
    }
    if (t < 3) {
      sbox[t] = NCELL;
      sbox[3 + t] = -1;
    }
    __syncthreads();
    if (act)
#pragma unroll
      for (int a = 0; a < 3; ++a) {
        atomicMin(&sbox[a], lo3[a]);
        atomicMax(&sbox[3 + a], hi3[a]);
      }
    __syncthreads();
    const int u0[3] = {sbox[0], sbox[1], sbox[2]};
    const int bx = sbox[3] - u0[0] + 1, by = sbox[4] - u0[1] + 1, bz = sbox[5] - u0[2] + 1;
    // (a barrier: sbox is free for the next level)
    if (__syncthreads_count(!done) == 0) break;
    if (bx <= 0) continue;  // no lane walks this level
    if (act)
#pragma unroll
      for (int j = 0; j < K; ++j) {
        bd[j] = (double)INFINITY;
        bi[j] = INT_MAX;
      }

    const int64_t ncell = (int64_t)bx * by * bz;
    if (ncell <= CAP) {
      // the cells 2t and 2t + 1 of the union box, x fastest
      int st[2], len[2];
#pragma unroll
      for (int u = 0; u < 2; ++u) {
        const int ci = 2 * t + u;
        st[u] = len[u] = 0;
        if (ci < (int)ncell) {
          int s, e;
          cell_range(pkeys, N, u0[0] + ci % bx, u0[1] + (ci / bx) % by, u0[2] + ci / (bx * by), L,
                     s, e);
          st[u] = s;
          len[u] = e - s;
        }
      }
      int tot;
      const int ex = block_exclusive_scan(len[0] + len[1], wsum, tot);
      cstart[2 * t] = st[0];
      cstart[2 * t + 1] = st[1];
      cpre[2 * t] = ex;
      cpre[2 * t + 1] = ex + len[0];
      if (t == NT - 1) cpre[CAP] = tot;
      __syncthreads();
      // the lane's block in the box's coordinates
      const uint32_t l0[3] = {(uint32_t)(lo3[0] - u0[0]), (uint32_t)(lo3[1] - u0[1]),
                              (uint32_t)(lo3[2] - u0[2])};
      const uint32_t w3[3] = {(uint32_t)(hi3[0] - lo3[0]), (uint32_t)(hi3[1] - lo3[1]),
                              (uint32_t)(hi3[2] - lo3[2])};
      for (int base = 0; base < tot; base += CH) {
        const int cnt = min(CH, tot - base);
        for (int s = t; s < cnt; s += NT) {
          // the cell holding item base + s of the concatenated ranges: the
          // first ci with cpre[ci + 1] > off (empty cells are stepped over)
          const int off = base + s;
          int a = 0, z = CAP - 1;
          while (a < z) {
            const int m = (a + z) >> 1;
            if (cpre[m + 1] <= off) a = m + 1; else z = m;
          }
          srec[s] = prec[cstart[a] + (off - cpre[a])];
          scode[s] = (uint32_t)(a % bx) | ((uint32_t)((a / bx) % by) << 10) |
                     ((uint32_t)(a / (bx * by)) << 20);
        }
        __syncthreads();
        if (act)
#pragma unroll 4
          for (int r = 0; r < cnt; ++r) {
            const uint32_t code = scode[r];
            if ((code & 1023u) - l0[0] <= w3[0] && ((code >> 10) & 1023u) - l0[1] <= w3[1] &&
                (code >> 20) - l0[2] <= w3[2]) {
              const float4 p = srec[r];
              consider(bd, bi, dist2(qd[0], qd[1], qd[2], p), __float_as_int(p.w));
            }
          }
        __syncthreads();
      }
    } else if (act) {
      for (int z = lo3[2]; z <= hi3[2]; ++z)
        for (int y = lo3[1]; y <= hi3[1]; ++y)
          for (int x = lo3[0]; x <= hi3[0]; ++x) {
            int s, e;
            cell_range(pkeys, N, x, y, z, L, s, e);
            for (int i = s; i < e; ++i) {
              const float4 p = prec[i];
              consider(bd, bi, dist2(qd[0], qd[1], qd[2], p), __float_as_int(p.w));
            }
          }
    }

    if (act) {
      double kth = bd[0], b2 = (double)INFINITY;
#pragma unroll
      for (int j = 1; j < K; ++j) kth = j == k - 1 ? bd[j] : kth;
      const double scale = (double)(1 << L);
#pragma unroll
      for (int a = 0; a < 3; ++a)
        if (b.inv[a] != 0.0)  // an axis without extent has one cell: no face
          b2 = fmin(b2, face_bound2(qd[a], b.lo[a], b.edge[a] * scale, b.margin[a], c[a] >> L, nc));
      if (L == LV || kth < b2) {
        done = true;
        const int64_t row = (int64_t)__float_as_int(q.w) * k;
#pragma unroll
        for (int j = 0; j < K; ++j)
          if (j < k) {
            dists[row + j] = (float)sqrt(bd[j]);
            // (a list that non-finite input left short: any index in range)
            idx[row + j] = bi[j] < N ? bi[j] : 0;
          }
      }
    }
  }
}

// The records (and keys) of n points sorted by Morton key, through the shared
// pair buffers (k0, v0, k1, v1).
inline void sort_cloud(const float *pts, int64_t n, const Box *box, uint32_t *k0, int32_t *v0,
                       uint32_t *k1, int32_t *v1, void *scratch, float4 *rec, uint64_t *keys,
                       hipStream_t st) {
  const dim3 grid((unsigned)((n + NT - 1) / NT)), blk(NT);
  hipLaunchKernelGGL(keys_lo_kernel, grid, blk, 0, st, pts, n, box, k0, v0);
  // 30 bits = 4 passes: the result is back where it started
  const int r0 = lsd_sort_pairs(k0, v0, k1, v1, n, 0, 30, scratch, st);
  const int32_t *perm = r0 ? v1 : v0;
  uint32_t *ka = r0 ? k0 : k1, *kb = r0 ? k1 : k0;
  int32_t *va = r0 ? v0 : v1, *vb = r0 ? v1 : v0;
  hipLaunchKernelGGL(keys_hi_kernel, grid, blk, 0, st, pts, n, box, perm, ka, va);
  const int r1 = lsd_sort_pairs(ka, va, kb, vb, n, 0, 30, scratch, st);
  hipLaunchKernelGGL(gather_kernel, grid, blk, 0, st, pts, n, box, r1 ? vb : va, rec, keys);
}

inline size_t align256(size_t x) { return (x + 255) & ~(size_t)255; }

// box partials | Box | k0 v0 k1 v1 | sort scratch | point records | point
// keys | query records
struct Workspace {
  size_t partial, box, pair[4], scratch, prec, pkeys, qrec, total;
  Workspace(int64_t N, int64_t M) {
    const int64_t nmax = std::max(N, M);
    size_t o = 0;
    auto take = [&o](size_t bytes) { const size_t at = o; o += align256(bytes); return at; };
    partial = take((size_t)BOX_BLOCKS * 6 * 4);
    box = take(sizeof(Box));
    for (size_t &p : pair) p = take((size_t)nmax * 4);
    // (the sort's tile size steps down past 2^20 items: not monotone in n)
    scratch = take(std::max(lsd_sort_scratch_bytes(N), lsd_sort_scratch_bytes(std::max<int64_t>(M, 1))));
    prec = take((size_t)N * 16);
    pkeys = take((size_t)N * 8);
    qrec = take((size_t)M * 16);
    total = o;
  }
};

}  // namespace knn
}  // namespace gs

using namespace gs;

// M = 0: the queries are the points themselves
extern "C" int64_t gsplat_hip_knn_workspace_bytes(int64_t N, int64_t M) {
  if (N < 1 || N > knn::MAX_POINTS || M < 0 || M > knn::MAX_POINTS) return 0;
  return (int64_t)knn::Workspace(N, M).total;
}

extern "C" int gsplat_hip_knn(int64_t N, const float *points, int64_t M, const float *queries,
                              int k, float *dists, int64_t *idx, void *workspace, void *stream) {
  GS_REQUIRE(N >= 1 && N <= knn::MAX_POINTS, "knn: N %lld outside [1, 2^30]", (long long)N);
  GS_REQUIRE(k >= 1 && k <= 32 && k <= N, "knn: k %d outside [1, min(32, N = %lld)]", k,
             (long long)N);
  GS_REQUIRE(points && dists && idx && workspace, "knn: null pointer");
  if (!queries) M = 0;
  GS_REQUIRE(M >= 0 && M <= knn::MAX_POINTS, "knn: M %lld outside [0, 2^30]", (long long)M);
  GS_REQUIRE(((uintptr_t)workspace & 15) == 0, "knn: workspace must be 16-B aligned");
  if (queries && M == 0) return 0;
  hipStream_t st = (hipStream_t)stream;
  const knn::Workspace w(N, M);
  char *base = reinterpret_cast<char *>(workspace);
  float *partial = reinterpret_cast<float *>(base + w.partial);
  knn::Box *box = reinterpret_cast<knn::Box *>(base + w.box);
  uint32_t *k0 = reinterpret_cast<uint32_t *>(base + w.pair[0]);
  int32_t *v0 = reinterpret_cast<int32_t *>(base + w.pair[1]);
  uint32_t *k1 = reinterpret_cast<uint32_t *>(base + w.pair[2]);
  int32_t *v1 = reinterpret_cast<int32_t *>(base + w.pair[3]);
  void *scratch = base + w.scratch;
  float4 *prec = reinterpret_cast<float4 *>(base + w.prec);
  uint64_t *pkeys = reinterpret_cast<uint64_t *>(base + w.pkeys);
  float4 *qrec = queries ? reinterpret_cast<float4 *>(base + w.qrec) : prec;

  const int nb = (int)std::min<int64_t>((N + knn::NT - 1) / knn::NT, knn::BOX_BLOCKS);
  hipLaunchKernelGGL(knn::box_partial_kernel, dim3(nb), dim3(knn::NT), 0, st, points, N, partial);
  hipLaunchKernelGGL(knn::box_final_kernel, dim3(1), dim3(knn::NT), 0, st, partial, nb, box);
  knn::sort_cloud(points, N, box, k0, v0, k1, v1, scratch, prec, pkeys, st);
  if (queries) knn::sort_cloud(queries, M, box, k0, v0, k1, v1, scratch, qrec, nullptr, st);
  const int64_t nq = queries ? M : N;
  const dim3 grid((unsigned)((nq + knn::NT - 1) / knn::NT)), blk(knn::NT);
#define GS_KNN_SEARCH(K)                                                                    \
  hipLaunchKernelGGL(knn::search_kernel<K>, grid, blk, 0, st, prec, pkeys, (int)N, qrec,    \
                     (int)nq, k, box, dists, idx)
  if (k <= 4) GS_KNN_SEARCH(4);
  else if (k <= 8) GS_KNN_SEARCH(8);
  else if (k <= 16) GS_KNN_SEARCH(16);
  else GS_KNN_SEARCH(32);
#undef GS_KNN_SEARCH
  GS_CHECK_LAUNCH("knn");
  return 0;
}
