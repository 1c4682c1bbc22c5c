// Splat compression (gsplat/compression/png_compression.py's _compress_kmeans:
// shN replaced by 65,536 centroids and a 16-bit label per Gaussian): the two
// passes of a Lloyd iteration with a Manhattan-distance assignment.
//
// Assignment:  labels[i] = argmin_k sum_d |x[i,d] - c[k,d]|, lowest k on a tie.
//   L1 distance is no GEMM, so this is a pure VALU kernel.  A lane keeps PPL = 2
//   point rows in VGPRs for the whole launch (a strided load, once; nothing
//   beside K * 2 D vector operations per point).  The workgroup streams the
//   centroids through LDS in tiles of TK rows, each row padded to a 16-byte
//   multiple; all lanes of a wave read the same address (`ds_read_b128`, a
//   broadcast: no bank conflict) and get four dimensions of one centroid per
//   read, worth 16 VALU operations (|.| is a source modifier: one subtract and
//   one add per dimension and point).  CG = 4 centroids x 2 points = 8
//   independent sums are in flight.  Every sum runs over d = 0 .. D-1 in order
//   in fp32 and centroids are compared in ascending k with a strict <: the
//   same input gives the same labels in every run.
//   The LDS tile is single-buffered between two barriers: a tile's fill is 24
//   dword loads per lane against ~23,000 VALU operations per wave (D = 45), and
//   the other workgroups of the CU (3 per CU at D = 45) cover it.
//   Built with -fno-slp-vectorize (Makefile): v_pk_add_f32 has no |.| modifier.
//
// Update:  c[k] = mean of the rows labelled k; a centroid without members keeps
//   its value; counts[k] = members.  Bit-reproducible, no float atomics: the
//   point ids are sorted by label (lsd_sort.h: stable, so ids ascend inside a
//   label), one wave per centroid finds its segment by binary search and adds
//   the segment's rows in order, a lane per dimension, in double (a mean of
//   terms of both signs must not lose what the fp32 sum would cancel).
#include "lsd_sort.h"

namespace gs {
namespace kmeansk {

constexpr int NT = 256;   // lanes per workgroup
constexpr int PPL = 2;    // point rows per lane
constexpr int TK = 128;   // centroid rows per LDS tile
constexpr int CG = 4;     // centroids in flight per point
constexpr int MAX_D = 72;
static_assert(TK % CG == 0, "a centroid group never leaves the tile");

// DT: the compiled row length.  PAD = false: D == DT exactly.  PAD = true: any
// D <= DT, the dimensions past D read as zero on both sides (|0 - 0| adds an
// exact 0, so the sums are those of the D dimensions alone).
// The point rows take 2 * DS registers, the two steps of centroid values in
// flight 32, the sums 8.  The budget is set so that 4, 3 or 2 waves share a
// SIMD without a spill (one wave alone issues a VALU instruction every 4
// cycles, two or more every 2).
constexpr int waves_per_simd(int dt) { return dt <= 16 ? 4 : dt <= 32 ? 3 : 2; }

template <int DT, bool PAD>
__global__ void __launch_bounds__(NT) __attribute__((amdgpu_waves_per_eu(waves_per_simd(DT))))
assign_kernel(int64_t N, int K, int D, const float *__restrict__ x, const float *__restrict__ c,
              int32_t *__restrict__ labels, float *__restrict__ dist,
              int32_t *__restrict__ n_changed) {
  constexpr int DS = (DT + 3) / 4 * 4;  // LDS row: a 16-byte multiple
  __shared__ __attribute__((aligned(16))) float tile[TK * DS];
  const int Dr = PAD ? D : DT;
  const int tid = threadIdx.x;

  float xr[PPL][DS];
  int64_t pi[PPL];
#pragma unroll
  for (int p = 0; p < PPL; ++p) {
    pi[p] = (int64_t)blockIdx.x * (NT * PPL) + p * NT + tid;
    const float *row = x + (pi[p] < N ? pi[p] : N - 1) * Dr;  // past N: a valid row, not stored
#pragma unroll
    for (int d = 0; d < DS; ++d) xr[p][d] = d < Dr ? row[d] : 0.f;
  }
  float best[PPL];
  int bl[PPL];
#pragma unroll
  for (int p = 0; p < PPL; ++p) best[p] = INFINITY, bl[p] = 0;

  for (int k0 = 0; k0 < K; k0 += TK) {
    __syncthreads();  // the previous tile has been read
    for (int e = tid; e < TK * DS; e += NT) {
      const int r = e / DS, col = e - r * DS, k = k0 + r;
      // a row past K is +inf: its distance is +inf, which a strict < never takes
      tile[e] = k < K ? (col < Dr ? c[(int64_t)k * Dr + col] : 0.f) : INFINITY;
    }
    __syncthreads();
    const int kt = min(TK, K - k0);
    for (int c0 = 0; c0 < kt; c0 += CG) {
      float acc[PPL][CG];
#pragma unroll
      for (int p = 0; p < PPL; ++p)
#pragma unroll
        for (int q = 0; q < CG; ++q) acc[p][q] = 0.f;
      const float4 *rows = reinterpret_cast<const float4 *>(tile + c0 * DS);
      // four dimensions of the CG centroids per step; the next step's reads are
      // issued before this step's arithmetic and nothing moves across a step
      // (left to itself the scheduler hoists every read of the group and
      // spills the point rows)
      float4 cur[CG], nxt[CG];
#pragma unroll
      for (int q = 0; q < CG; ++q) cur[q] = rows[q * (DS / 4)];
#pragma unroll
      for (int g = 0; g < DS / 4; ++g) {
        if (g + 1 < DS / 4) {
#pragma unroll
          for (int q = 0; q < CG; ++q) nxt[q] = rows[q * (DS / 4) + g + 1];
        }
#pragma unroll
        for (int q = 0; q < CG; ++q) {
          const float v[4] = {cur[q].x, cur[q].y, cur[q].z, cur[q].w};
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            if (4 * g + j >= DT) continue;
#pragma unroll
            for (int p = 0; p < PPL; ++p) acc[p][q] += fabsf(xr[p][4 * g + j] - v[j]);
          }
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int q = 0; q < CG; ++q) cur[q] = nxt[q];
      }
#pragma unroll
      for (int q = 0; q < CG; ++q) {
        const int k = k0 + c0 + q;
#pragma unroll
        for (int p = 0; p < PPL; ++p) {
          const bool lt = acc[p][q] < best[p];
          best[p] = lt ? acc[p][q] : best[p];
          bl[p] = lt ? k : bl[p];
        }
      }
    }
  }

  int changed = 0;
#pragma unroll
  for (int p = 0; p < PPL; ++p) {
    bool ch = false;
    if (pi[p] < N) {
      ch = labels[pi[p]] != bl[p];
      labels[pi[p]] = bl[p];
      if (dist) dist[pi[p]] = best[p];
    }
    changed += __popcll(__ballot(ch));
  }
  if (n_changed && changed && (tid & 63) == 0) atomicAdd(n_changed, changed);
}

__global__ void __launch_bounds__(256)
sort_keys_kernel(int64_t N, const int32_t *__restrict__ labels, uint32_t *__restrict__ keys,
                 int32_t *__restrict__ ids) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= N) return;
  keys[i] = (uint32_t)labels[i];
  ids[i] = (int32_t)i;
}

// first position in the ascending keys[0, n) holding a key >= k
GS_INLINE int64_t lower_bound(const uint32_t *__restrict__ keys, int64_t n, uint32_t k) {
  int64_t lo = 0, hi = n;
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if (keys[mid] < k) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// One wave per centroid; lane l sums dimensions l and l + 64.
__global__ void __launch_bounds__(256)
mean_kernel(int64_t N, int K, int D, const float *__restrict__ x,
            const uint32_t *__restrict__ keys, const int32_t *__restrict__ ids,
            float *__restrict__ c, int32_t *__restrict__ counts) {
  const int k = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (k >= K) return;
  const int64_t s = lower_bound(keys, N, (uint32_t)k);
  const int64_t e = lower_bound(keys, N, (uint32_t)k + 1u);
  if (lane == 0) counts[k] = (int32_t)(e - s);
  if (e <= s) return;  // no members: the centroid stays
  const bool two = lane + 64 < D;
  const int d0 = lane < D ? lane : 0;  // an idle lane reads dimension 0, stores nothing
  const int d1 = two ? lane + 64 : 0;
  double s0 = 0.0, s1 = 0.0;
  for (int64_t j = s; j < e; ++j) {
    const float *row = x + (int64_t)ids[j] * D;
    s0 += (double)row[d0];
    s1 += (double)row[d1];
  }
  const double n = (double)(e - s);
  if (lane < D) c[(int64_t)k * D + lane] = (float)(s0 / n);
  if (two) c[(int64_t)k * D + lane + 64] = (float)(s1 / n);
}

inline int64_t align16(int64_t b) { return (b + 15) & ~(int64_t)15; }

// bits of the largest label K - 1 (0 for K = 1: nothing to sort)
inline int label_bits(int K) {
  int b = 0;
  while (b < 16 && (1 << b) < K) ++b;
  return b;
}

}  // namespace kmeansk
}  // namespace gs

using namespace gs;

static int kmeans_check(const char *who, int64_t N, int K, int D) {
  GS_REQUIRE(N >= 1 && N < ((int64_t)1 << 31), "%s: N %lld outside [1, 2^31)", who, (long long)N);
  GS_REQUIRE(K >= 1 && K <= 65536, "%s: K %d outside [1, 65536]", who, K);
  GS_REQUIRE(D >= 1 && D <= kmeansk::MAX_D, "%s: D %d outside [1, %d]", who, D, kmeansk::MAX_D);
  return 0;
}

extern "C" int gsplat_hip_kmeans_l1_assign(int64_t N, int K, int D, const float *x,
                                           const float *centroids, int32_t *labels, float *dist,
                                           int32_t *n_changed, void *stream) {
  if (int rc = kmeans_check("kmeans_l1_assign", N, K, D)) return rc;
  GS_REQUIRE(x && centroids && labels, "kmeans_l1_assign: null pointer");
  hipStream_t st = (hipStream_t)stream;
  if (n_changed) GS_HIP(zero_async(n_changed, sizeof(int32_t), st));
  const int64_t per = kmeansk::NT * kmeansk::PPL;
  const dim3 grid((unsigned)((N + per - 1) / per)), block(kmeansk::NT);
#define GS_KMEANS_ASSIGN(DT, PAD)                                                              \
  hipLaunchKernelGGL((kmeansk::assign_kernel<DT, PAD>), grid, block, 0, st, N, K, D, x,        \
                     centroids, labels, dist, n_changed)
  // shN of degrees 1-3 at their exact length, anything else in the next size up
  if (D == 9) GS_KMEANS_ASSIGN(9, false);
  else if (D == 24) GS_KMEANS_ASSIGN(24, false);
  else if (D == 45) GS_KMEANS_ASSIGN(45, false);
  else if (D <= 8) GS_KMEANS_ASSIGN(8, true);
  else if (D <= 16) GS_KMEANS_ASSIGN(16, true);
  else if (D <= 32) GS_KMEANS_ASSIGN(32, true);
  else if (D <= 48) GS_KMEANS_ASSIGN(48, true);
  else if (D <= 64) GS_KMEANS_ASSIGN(64, true);
  else GS_KMEANS_ASSIGN(72, true);
#undef GS_KMEANS_ASSIGN
  GS_CHECK_LAUNCH("kmeans_l1_assign");
  return 0;
}

// keys / ids, twice (the sort's ping-pong), then the sort's scratch
extern "C" int64_t gsplat_hip_kmeans_update_workspace_bytes(int64_t N) {
  if (N < 1 || N >= ((int64_t)1 << 31)) return 0;
  return 4 * kmeansk::align16(4 * N) + kmeansk::align16((int64_t)lsd_sort_scratch_bytes(N));
}

extern "C" int gsplat_hip_kmeans_update(int64_t N, int K, int D, const float *x,
                                        const int32_t *labels, float *centroids, int32_t *counts,
                                        void *workspace, void *stream) {
  if (int rc = kmeans_check("kmeans_update", N, K, D)) return rc;
  GS_REQUIRE(x && labels && centroids && counts && workspace, "kmeans_update: null pointer");
  GS_REQUIRE(((uintptr_t)workspace & 15) == 0, "kmeans_update: workspace must be 16-B aligned");
  hipStream_t st = (hipStream_t)stream;
  char *w = reinterpret_cast<char *>(workspace);
  const int64_t a = kmeansk::align16(4 * N);
  uint32_t *k0 = reinterpret_cast<uint32_t *>(w), *k1 = reinterpret_cast<uint32_t *>(w + 2 * a);
  int32_t *v0 = reinterpret_cast<int32_t *>(w + a), *v1 = reinterpret_cast<int32_t *>(w + 3 * a);
  hipLaunchKernelGGL(kmeansk::sort_keys_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0,
                     st, N, labels, k0, v0);
  const int cur = lsd_sort_pairs(k0, v0, k1, v1, N, 0, kmeansk::label_bits(K), w + 4 * a, st);
  hipLaunchKernelGGL(kmeansk::mean_kernel, dim3((unsigned)((K + 3) / 4)), dim3(256), 0, st, N, K,
                     D, x, cur ? k1 : k0, cur ? v1 : v0, centroids, counts);
  GS_CHECK_LAUNCH("kmeans_update");
  return 0;
}
