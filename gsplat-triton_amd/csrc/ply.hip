// PLY rows in the INRIA layout for gfx950 (gsplat/utils.py:10-98 save_ply):
// the Gaussians' parameters (structure of arrays) packed into the file's
// vertex rows, rows with a non-finite field dropped, and the way back.
//
//   row = x y z | nx ny nz (0) | f_dc_0..2 | f_rest_0..R-1 | opacity | scale_0..2 | rot_0..3
//   F   = 17 + R floats, R = 3 K1, K1 = the shN coefficients per channel
//   f_rest_j = shN[n, j % K1, j / K1]   (channel-major: shN.transpose(0, 2, 1))
//   with colours: R = 0 and f_dc_j = (colors[n, j] - 0.5) / C0, an fp32
//   subtract and a correctly rounded fp32 divide by the fp32 constant
//
// count:  one workgroup per 256 source rows.  Its fields are walked as the
//         contiguous spans they are (coalesced); a non-finite value marks its
//         row in LDS.  Then one lane per row: the row's validity byte, and the
//         workgroup's kept rows by wave ballots.  The exclusive scan of the
//         per-workgroup counts is projection.hip's launch_packed_scan.
// pack:   the kept rows of a workgroup are one contiguous span of the output,
//         [off, off + kept) * F: lane e of the span writes float e (coalesced)
//         and finds its source through the kept-rank -> row table in LDS.  The
//         shN transposition reads stride-3 inside the row's own cache lines.
// unpack: lane e = (row, property) reads rows[row, cols[property]] and writes
//         the parameter arrays (shN transposed back).  No compaction.
// No atomics on global memory, every store a plain vector store.
#include <math.h>

#include "common.h"
#include "proj_math.h"  // launch_packed_scan

namespace gs {
namespace ply {

constexpr int kRows = 256;                 // source rows per workgroup
constexpr float kC0 = 0.2820947917738781f; // SH band 0, rounded to fp32

struct Src {
  const float *means, *scales, *quats, *opacities, *sh0, *shN, *colors;
  int64_t n;
  int K1;  // shN coefficients per channel (0 with colours)
};

GS_INLINE float f_dc_of_color(float c) { return __fdiv_rn(__fsub_rn(c, 0.5f), kC0); }

// marks bad[r] for every row r of the workgroup with a non-finite value among
// the `width` floats per row of `p` (rows row0 .. row0 + nr)
template <bool COLOR>
GS_INLINE void scan_field(const float *p, int width, int64_t row0, int nr, int *bad) {
  if (!p || width == 0) return;
  const float *q = p + row0 * width;
  const int total = nr * width;
  for (int e = threadIdx.x; e < total; e += kRows) {
    float v = q[e];
    if (COLOR) v = f_dc_of_color(v);
    if (!isfinite(v)) bad[e / width] = 1;
  }
}

__global__ void __launch_bounds__(kRows) count_kernel(Src a, int64_t *block_cnt, uint8_t *valid) {
  __shared__ int bad[kRows];
  __shared__ int wave_cnt[4];
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int nr = a.n - row0 < kRows ? (int)(a.n - row0) : kRows;
  bad[threadIdx.x] = 0;
  __syncthreads();
  scan_field<false>(a.means, 3, row0, nr, bad);
  scan_field<false>(a.scales, 3, row0, nr, bad);
  scan_field<false>(a.quats, 4, row0, nr, bad);
  scan_field<false>(a.opacities, 1, row0, nr, bad);
  if (a.colors) {
    scan_field<true>(a.colors, 3, row0, nr, bad);
  } else {
    scan_field<false>(a.sh0, 3, row0, nr, bad);
    scan_field<false>(a.shN, 3 * a.K1, row0, nr, bad);
  }
  __syncthreads();
  const bool keep = (int)threadIdx.x < nr && !bad[threadIdx.x];
  if ((int)threadIdx.x < nr) valid[row0 + threadIdx.x] = keep ? 1 : 0;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t m = __ballot(keep);
  if (lane == 0) wave_cnt[wid] = __popcll(m);
  __syncthreads();
  if (threadIdx.x == 0)
    block_cnt[blockIdx.x] = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
}

// the float of column `col` of source row `row`
GS_INLINE float field_at(const Src &a, int64_t row, int col) {
  const int R = 3 * a.K1;
  if (col < 3) return a.means[3 * row + col];
  if (col < 6) return 0.f;
  if (col < 9) {
    const int j = col - 6;
    return a.colors ? f_dc_of_color(a.colors[3 * row + j]) : a.sh0[3 * row + j];
  }
  if (col < 9 + R) {
    const int j = col - 9, c = j / a.K1, k = j - c * a.K1;
    return a.shN[(int64_t)R * row + 3 * k + c];
  }
  col -= 9 + R;
  if (col == 0) return a.opacities[row];
  if (col < 4) return a.scales[3 * row + col - 1];
  return a.quats[4 * row + col - 4];
}

__global__ void __launch_bounds__(kRows) pack_kernel(Src a, const int64_t *block_off,
                                                     const uint8_t *valid, float *rows) {
  __shared__ int src_of[kRows];
  __shared__ int wave_cnt[4];
  const int64_t row0 = (int64_t)blockIdx.x * kRows;
  const int nr = a.n - row0 < kRows ? (int)(a.n - row0) : kRows;
  const bool keep = (int)threadIdx.x < nr && valid[row0 + threadIdx.x] != 0;
  const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
  const uint64_t m = __ballot(keep);
  if (lane == 0) wave_cnt[wid] = __popcll(m);
  __syncthreads();
  int before = 0;
  for (int w = 0; w < wid; ++w) before += wave_cnt[w];
  if (keep)
    src_of[before + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                              __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0))] =
        threadIdx.x;
  __syncthreads();
  const int kept = wave_cnt[0] + wave_cnt[1] + wave_cnt[2] + wave_cnt[3];
  const int F = 17 + 3 * a.K1;
  float *out = rows + block_off[blockIdx.x] * F;
  const int total = kept * F;  // <= 256 * 89
  for (int e = threadIdx.x; e < total; e += kRows) {
    const int r = e / F, col = e - r * F;
    out[e] = field_at(a, row0 + src_of[r], col);
  }
}

struct Dst {
  float *means, *scales, *quats, *opacities, *sh0, *shN;
  int64_t n;
  int K1, F;  // F: floats per file row
};

__global__ void __launch_bounds__(256) unpack_kernel(Dst a, const float *rows,
                                                     const int32_t *cols) {
  const int R = 3 * a.K1, P = 14 + R;
  const int64_t total = a.n * P;
  const int64_t stride = (int64_t)gridDim.x * 256;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += stride) {
    const int64_t row = e / P;
    int p = (int)(e - row * P);
    const float v = rows[row * a.F + cols[p]];
    if (p < 3) {
      a.means[3 * row + p] = v;
    } else if (p < 6) {
      a.sh0[3 * row + p - 3] = v;
    } else if (p < 6 + R) {
      const int j = p - 6, c = j / a.K1, k = j - c * a.K1;
      a.shN[(int64_t)R * row + 3 * k + c] = v;
    } else {
      p -= 6 + R;
      if (p == 0) a.opacities[row] = v;
      else if (p < 4) a.scales[3 * row + p - 1] = v;
      else a.quats[4 * row + p - 4] = v;
    }
  }
}

constexpr int64_t kMaxRows = (int64_t)1 << 31;  // per call: the grid and the int offsets

static int64_t blocks_of(int64_t n) { return (n + kRows - 1) / kRows; }
// the validity bytes follow the per-workgroup counts, 16-B aligned
static int64_t valid_offset(int64_t n) { return (blocks_of(n) * 8 + 15) / 16 * 16; }

static int check_src(const char *who, int64_t n, int K1, const Src &a) {
  GS_REQUIRE(n >= 0 && n <= kMaxRows, "%s: n=%lld not in 0..2^31", who, (long long)n);
  GS_REQUIRE(K1 >= 0 && K1 <= 24, "%s: K1=%d not in 0..24", who, K1);
  if (n == 0) return 0;
  GS_REQUIRE(a.means && a.scales && a.quats && a.opacities, "%s: null pointer argument", who);
  if (a.colors) {
    GS_REQUIRE(K1 == 0, "%s: colours take no shN (K1=%d)", who, K1);
  } else {
    GS_REQUIRE(a.sh0 && (K1 == 0 || a.shN), "%s: null sh0 / shN", who);
  }
  return 0;
}

}  // namespace ply
}  // namespace gs

using namespace gs;
using namespace gs::ply;

extern "C" int64_t gsplat_hip_ply_workspace_bytes(int64_t n) {
  if (n < 0) return 0;
  return valid_offset(n) + (n + 15) / 16 * 16;
}

extern "C" int gsplat_hip_ply_count(int64_t n, int K1, const float *means, const float *scales,
                                    const float *quats, const float *opacities, const float *sh0,
                                    const float *shN, const float *colors, void *workspace,
                                    int64_t *n_valid_device, void *stream) {
  Src a{means, scales, quats, opacities, sh0, shN, colors, n, K1};
  if (int rc = check_src("ply_count", n, K1, a)) return rc;
  GS_REQUIRE(n_valid_device, "ply_count: null n_valid_device");
  hipStream_t st = (hipStream_t)stream;
  if (n == 0) {
    GS_HIP(gs::zero_async(n_valid_device, sizeof(int64_t), st));
    return 0;
  }
  GS_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 && ((uintptr_t)n_valid_device & 7) == 0,
             "ply_count: workspace and n_valid_device must be 8-B aligned");
  int64_t *cnt = reinterpret_cast<int64_t *>(workspace);
  uint8_t *valid = reinterpret_cast<uint8_t *>(workspace) + valid_offset(n);
  const int64_t nb = blocks_of(n);
  hipLaunchKernelGGL(count_kernel, dim3((unsigned)nb), dim3(kRows), 0, st, a, cnt, valid);
  gs::launch_packed_scan(nb, cnt, n_valid_device, st);
  GS_CHECK_LAUNCH("ply_count");
  return 0;
}

extern "C" int gsplat_hip_ply_pack(int64_t n, int K1, const float *means, const float *scales,
                                   const float *quats, const float *opacities, const float *sh0,
                                   const float *shN, const float *colors, const void *workspace,
                                   float *rows, void *stream) {
  Src a{means, scales, quats, opacities, sh0, shN, colors, n, K1};
  if (int rc = check_src("ply_pack", n, K1, a)) return rc;
  if (n == 0) return 0;
  GS_REQUIRE(workspace && ((uintptr_t)workspace & 7) == 0 && rows,
             "ply_pack: null rows or workspace, or a workspace that is not 8-B aligned");
  const int64_t *off = reinterpret_cast<const int64_t *>(workspace);
  const uint8_t *valid = reinterpret_cast<const uint8_t *>(workspace) + valid_offset(n);
  hipLaunchKernelGGL(pack_kernel, dim3((unsigned)blocks_of(n)), dim3(kRows), 0,
                     (hipStream_t)stream, a, off, valid, rows);
  GS_CHECK_LAUNCH("ply_pack");
  return 0;
}

extern "C" int gsplat_hip_ply_unpack(int64_t n, int K1, int F, const float *rows,
                                     const int32_t *cols, float *means, float *scales,
                                     float *quats, float *opacities, float *sh0, float *shN,
                                     void *stream) {
  GS_REQUIRE(n >= 0 && n <= kMaxRows, "ply_unpack: n=%lld not in 0..2^31", (long long)n);
  GS_REQUIRE(K1 >= 0 && K1 <= 24, "ply_unpack: K1=%d not in 0..24", K1);
  GS_REQUIRE(F >= 14 + 3 * K1, "ply_unpack: F=%d below the %d named properties", F, 14 + 3 * K1);
  if (n == 0) return 0;
  GS_REQUIRE(rows && cols && means && scales && quats && opacities && sh0 && (K1 == 0 || shN),
             "ply_unpack: null pointer argument");
  Dst a{means, scales, quats, opacities, sh0, shN, n, K1, F};
  const int64_t total = n * (14 + 3 * K1);
  const int64_t blocks = std::min<int64_t>((total + 255) / 256, 1 << 16);
  hipLaunchKernelGGL(unpack_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)stream, a,
                     rows, cols);
  GS_CHECK_LAUNCH("ply_unpack");
  return 0;
}
