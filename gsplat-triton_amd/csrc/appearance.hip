// Appearance optimisation for the 3DGS trainer (examples/utils.py
// AppearanceOptModule, simple_trainer.py app_opt), for gfx950.
//
//   x      = cat(embeds[id[c]] (16), features[n] (32), sh_bases(normalize(means[n] - campos[c])) (16))
//   colors = sigmoid(W3 relu(W2 relu(W1 x + b1) + b2) + b3 + base_colors[n])
//
// Both 64x64 layers run on the f32-input MFMA (v_mfma_f32_32x32x2_f32: an
// exact k-ordered fp32 fma chain).  The products are taken transposed,
// Y^T[unit][row] = W[unit][k] X^T[k][row], so the weights are the A operand
// (read from LDS) and a row of activations stays on one lane pair: the
// accumulator of one layer -- column (= Gaussian) on the lane, units in the 16
// registers -- is the B operand of the next with no lane movement and no LDS.
// The k order inside a layer is the accumulator's register order, not 0..63;
// the A operand is read in that same order.
//
//   app_fwd_kernel     colours, 128 rows per workgroup pass (32 per wave)
//   app_bwd_kernel     recomputes the activations; per-row gradients in place,
//                      weight gradients as MFMA products dW = dZ X^T over
//                      wave-private LDS transposes, summed in registers over
//                      the workgroup's rows, one workspace row per workgroup
//   app_reduce_kernel  ordered sum of the workspace rows
//   app_adam_kernel    torch.optim.Adam on the head and (with L2 decay, dense)
//                      on the embedding table
// No floating-point atomics anywhere: every sum has a fixed order.
#include <atomic>
#include "common.h"
#include "sh_basis.h"
#include "../../include/gsplat_hip.h"

namespace gs {

typedef float f32x16 __attribute__((ext_vector_type(16)));

constexpr int kAppW = 64;        // input and hidden width
constexpr int kAppEmbed = 16;
constexpr int kAppFeat = 32;
constexpr int kAppBases = 16;
constexpr int kAppLd = 65;       // LDS row stride of a weight matrix (banks)
constexpr int kAppTile = 128;    // rows per workgroup pass
constexpr int kAppWaveRows = 32;
constexpr int kAppMaxGrid = 256; // persistent grid: one workgroup per CU
constexpr int kAppSt = 68;       // row stride of a staged [row][unit] tile
constexpr float kAppNormEps = 1e-12f;  // F.normalize's clamp

// flat order of the head's gradients (torch Linear layout), then 16 per camera
constexpr int kOffW1 = 0, kOffB1 = 4096, kOffW2 = 4160, kOffB2 = 8256, kOffW3 = 8320,
              kOffB3 = 8512, kAppHead = 8515;

struct AppHead {
  const float *W1, *b1, *W2, *b2, *W3, *b3;
};

struct AppIn {
  int C;
  int64_t N;
  int nb;  // bases in use, (deg + 1)^2
  const float *means, *campos, *features, *base;
  const float *embeds;       // [n_images, 16] or null
  const int64_t *embed_ids;  // [C] or null
  int n_images;
  AppHead hd;
  const uint8_t *masks;   // [C, N] or null
  const int32_t *radii;   // [C, N] or null (> 0 = visible)
};

// shared-memory image of the head: W1, W2 with padded rows, then the rest
constexpr int kLdsW1 = 0, kLdsW2 = kAppW * kAppLd, kLdsW3 = 2 * kAppW * kAppLd,
              kLdsB1 = kLdsW3 + 3 * kAppW, kLdsB2 = kLdsB1 + kAppW, kLdsB3 = kLdsB2 + kAppW,
              kLdsHead = kLdsB3 + 4;
// per wave: two staged tiles and the three colour gradients of its 32 rows
constexpr int kLdsWave = 2 * kAppWaveRows * kAppSt + 3 * kAppWaveRows;

GS_INLINE void load_head(const AppHead &hd, float *s) {
  for (int e = threadIdx.x; e < kAppW * kAppW; e += blockDim.x) {
    const int r = e >> 6, c = e & 63;
    s[kLdsW1 + r * kAppLd + c] = hd.W1[e];
    s[kLdsW2 + r * kAppLd + c] = hd.W2[e];
  }
  for (int e = threadIdx.x; e < 3 * kAppW; e += blockDim.x) s[kLdsW3 + e] = hd.W3[e];
  if (threadIdx.x < kAppW) {
    s[kLdsB1 + threadIdx.x] = hd.b1[threadIdx.x];
    s[kLdsB2 + threadIdx.x] = hd.b2[threadIdx.x];
  }
  if (threadIdx.x < 3) s[kLdsB3 + threadIdx.x] = hd.b3[threadIdx.x];
}

// the unit (row of the transposed product) that register r of accumulator
// tile t holds on lane half h: the 32x32 C/D map, row = (r&3) + 8 (r>>2) + 4 h
GS_INLINE constexpr int acc_unit(int r, int h, int t) {
  return 32 * t + (r & 3) + 8 * (r >> 2) + 4 * h;
}

// lanes of one wave exchange data through their private LDS region
GS_INLINE void wave_lds_sync() {
  __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "workgroup");
  __builtin_amdgcn_wave_barrier();
}

GS_INLINE int64_t app_embed_row(const AppIn &a, int c) {
  const int64_t i = a.embed_ids[c];
  return i < 0 ? 0 : (i >= a.n_images ? (int64_t)a.n_images - 1 : i);
}

// One lane's share of one row of the input: lane half h of the pair that owns
// the row holds embed 8h.., features 16h.., bases 8h..
struct AppRow {
  float xe[8], xf[16], xb[8];
  float dir[3], len;  // normalised direction, |means - campos|
  bool valid;
};

template <bool GRAD>
GS_INLINE void app_load_row(const AppIn &a, int c, int64_t row, int h, AppRow &x,
                            float (*dB)[3]) {
  x.valid = row < a.N;
  if (x.valid && a.masks) x.valid = a.masks[(int64_t)c * a.N + row] != 0;
  if (x.valid && a.radii) x.valid = a.radii[(int64_t)c * a.N + row] > 0;
  const bool emb = a.embeds && a.embed_ids;
  const float *e = emb ? a.embeds + app_embed_row(a, c) * kAppEmbed + 8 * h : nullptr;
#pragma unroll
  for (int k = 0; k < 8; ++k) x.xe[k] = (emb && x.valid) ? e[k] : 0.f;
  float B[kAppBases];
  if (x.valid) {
    const float4 *f = reinterpret_cast<const float4 *>(a.features + row * kAppFeat + 16 * h);
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const float4 v = f[q];
      x.xf[4 * q] = v.x; x.xf[4 * q + 1] = v.y; x.xf[4 * q + 2] = v.z; x.xf[4 * q + 3] = v.w;
    }
    const float dx = a.means[3 * row] - a.campos[3 * c];
    const float dy = a.means[3 * row + 1] - a.campos[3 * c + 1];
    const float dz = a.means[3 * row + 2] - a.campos[3 * c + 2];
    x.len = sqrtf(dx * dx + dy * dy + dz * dz);
    const float inv = 1.f / fmaxf(x.len, kAppNormEps);
    x.dir[0] = dx * inv; x.dir[1] = dy * inv; x.dir[2] = dz * inv;
    sh_basis<3, GRAD>(x.dir[0], x.dir[1], x.dir[2], B, dB);
  } else {
#pragma unroll
    for (int k = 0; k < 16; ++k) x.xf[k] = 0.f;
#pragma unroll
    for (int k = 0; k < kAppBases; ++k) B[k] = 0.f;
    x.dir[0] = x.dir[1] = x.dir[2] = 0.f;
    x.len = 0.f;
    if (GRAD) {
#pragma unroll
      for (int k = 0; k < kAppBases; ++k) dB[k][0] = dB[k][1] = dB[k][2] = 0.f;
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const float lo = k < a.nb ? B[k] : 0.f, hi = k + 8 < a.nb ? B[k + 8] : 0.f;
    x.xb[k] = h ? hi : lo;
  }
}

// hidden layers 1 and 2 for the wave's 32 rows: H1, H2 (after the ReLU), in
// the accumulator layout
GS_INLINE void app_trunk(const float *s, const AppRow &x, int i, int h, f32x16 (&H1)[2],
                         f32x16 (&H2)[2]) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) H1[t][r] = s[kLdsB1 + acc_unit(r, h, t)];
  const float *w1 = s + kLdsW1;
#pragma unroll
  for (int st = 0; st < 32; ++st) {
    const int k = st < 8 ? 8 * h + st : (st < 24 ? 16 + 16 * h + (st - 8) : 48 + 8 * h + (st - 24));
    const float b = st < 8 ? x.xe[st] : (st < 24 ? x.xf[st - 8] : x.xb[st - 24]);
#pragma unroll
    for (int t = 0; t < 2; ++t)
      H1[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[(i + 32 * t) * kAppLd + k], b, H1[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      H1[t][r] = fmaxf(H1[t][r], 0.f);
      H2[t][r] = s[kLdsB2 + acc_unit(r, h, t)];
    }
  const float *w2 = s + kLdsW2;
#pragma unroll
  for (int st = 0; st < 32; ++st) {
    const int k = acc_unit(st & 15, h, st >> 4);
    const float b = H1[st >> 4][st & 15];
#pragma unroll
    for (int t = 0; t < 2; ++t)
      H2[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w2[(i + 32 * t) * kAppLd + k], b, H2[t], 0, 0, 0);
  }
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) H2[t][r] = fmaxf(H2[t][r], 0.f);
}

// the last layer and the sigmoid: both lanes of a pair end with the colour.
// The sigmoid of the fp32 logit is taken in double (three per row): the
// colour and its derivative then carry the logit's rounding only.
GS_INLINE void app_head_out(const float *s, const f32x16 (&H2)[2], int h, const float *base,
                            double *col) {
  float o[3] = {0.f, 0.f, 0.f};
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int u = acc_unit(r, h, t);
#pragma unroll
      for (int q = 0; q < 3; ++q) o[q] = __fmaf_rn(s[kLdsW3 + q * kAppW + u], H2[t][r], o[q]);
    }
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    // the same order of additions on both lanes: low half first
    const float other = __shfl_xor(o[q], 32, kWave);
    const float lo = h ? other : o[q], hi = h ? o[q] : other;
    const float z = (lo + hi) + s[kLdsB3 + q] + base[q];
    col[q] = 1.0 / (1.0 + exp(-(double)z));
  }
}

__global__ void __launch_bounds__(256) app_fwd_kernel(AppIn a, float *__restrict__ colors) {
  extern __shared__ __align__(16) float smem[];
  load_head(a.hd, smem);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, h = lane >> 5;
  const int64_t ntiles = (a.N + kAppTile - 1) / kAppTile;
  for (int c = 0; c < a.C; ++c)
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      const int64_t row = tile * kAppTile + wave * kAppWaveRows + i;
      AppRow x;
      app_load_row<false>(a, c, row, h, x, nullptr);
      double col[3] = {0.0, 0.0, 0.0};
      if (__any(x.valid)) {  // wave-uniform: a wave of invisible rows costs nothing
        f32x16 H1[2], H2[2];
        app_trunk(smem, x, i, h, H1, H2);
        float base[3] = {0.f, 0.f, 0.f};
        if (x.valid) {
          base[0] = a.base[3 * row]; base[1] = a.base[3 * row + 1]; base[2] = a.base[3 * row + 2];
        }
        app_head_out(smem, H2, h, base, col);
      }
      if (h == 0 && row < a.N) {
        float *o = colors + ((int64_t)c * a.N + row) * 3;
#pragma unroll
        for (int q = 0; q < 3; ++q) o[q] = x.valid ? (float)col[q] : 0.f;
      }
    }
}

// write an accumulator-layout tensor (32 units per lane) to a [row][unit] tile
GS_INLINE void app_stage(float *dst, const f32x16 (&A)[2], int i, int h) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int g = 0; g < 4; ++g)
      *reinterpret_cast<float4 *>(dst + i * kAppSt + acc_unit(4 * g, h, t)) =
          make_float4(A[t][4 * g], A[t][4 * g + 1], A[t][4 * g + 2], A[t][4 * g + 3]);
}

// dW[u][k] += sum over the wave's 32 rows of dZ[row][u] X[row][k]: A and B
// both read contiguously from the staged tiles; dW[mt][nt] holds unit
// acc_unit(r, h, mt) x input (lane & 31) + 32 nt
GS_INLINE void app_outer(const float *dz, const float *xin, int i, int h, f32x16 (&dW)[2][2]) {
#pragma unroll
  for (int st = 0; st < 16; ++st) {
    const int n = 2 * st + h;
    const float a0 = dz[n * kAppSt + i], a1 = dz[n * kAppSt + i + 32];
    const float b0 = xin[n * kAppSt + i], b1 = xin[n * kAppSt + i + 32];
    dW[0][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b0, dW[0][0], 0, 0, 0);
    dW[0][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b1, dW[0][1], 0, 0, 0);
    dW[1][0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b0, dW[1][0], 0, 0, 0);
    dW[1][1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b1, dW[1][1], 0, 0, 0);
  }
}

// dX[k][row] = sum_u W[u][k] dZ[u][row], dZ in the accumulator layout
GS_INLINE void app_back(const float *w, const f32x16 (&dZ)[2], int i, int h, f32x16 (&dX)[2]) {
#pragma unroll
  for (int t = 0; t < 2; ++t)
#pragma unroll
    for (int r = 0; r < 16; ++r) dX[t][r] = 0.f;
#pragma unroll
  for (int st = 0; st < 32; ++st) {
    const int u = acc_unit(st & 15, h, st >> 4);
    const float b = dZ[st >> 4][st & 15];
#pragma unroll
    for (int t = 0; t < 2; ++t)
      dX[t] = __builtin_amdgcn_mfma_f32_32x32x2f32(w[u * kAppLd + i + 32 * t], b, dX[t], 0, 0, 0);
  }
}

// the column sums of a staged tile: lane = unit
GS_INLINE double app_colsum(const float *t, int lane) {
  double s = 0.0;
#pragma unroll
  for (int n = 0; n < kAppWaveRows; ++n) s += t[n * kAppSt + lane];
  return s;
}

// sum of the four waves' 64x64 accumulators, through their LDS regions
GS_INLINE void app_reduce_tiles(float *stage, const f32x16 (&dW)[2][2], int wave, int i, int h,
                                float *out) {
  float *mine = stage + wave * kLdsWave;
  __syncthreads();
#pragma unroll
  for (int mt = 0; mt < 2; ++mt)
#pragma unroll
    for (int nt = 0; nt < 2; ++nt)
#pragma unroll
      for (int r = 0; r < 16; ++r) mine[acc_unit(r, h, mt) * kAppW + i + 32 * nt] = dW[mt][nt][r];
  __syncthreads();
  for (int e = threadIdx.x; e < kAppW * kAppW; e += blockDim.x)
    out[e] = ((stage[e] + stage[kLdsWave + e]) + stage[2 * kLdsWave + e]) + stage[3 * kLdsWave + e];
}

// sum of one value per lane (lane = unit) over the four waves
GS_INLINE void app_reduce_lanes(float *stage, double v, int count, int wave, int lane,
                                 float *out) {
  __syncthreads();
  reinterpret_cast<double *>(stage + wave * kLdsWave)[lane] = v;
  __syncthreads();
  if ((int)threadIdx.x < count) {
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < 4; ++w)
      t += reinterpret_cast<const double *>(stage + w * kLdsWave)[threadIdx.x];
    out[threadIdx.x] = (float)t;
  }
}

static_assert(kLdsWave >= kAppW * kAppW, "a wave's staging region holds one 64x64 accumulator");

__global__ void __launch_bounds__(256) app_bwd_kernel(AppIn a, const float *__restrict__ v_colors,
                                                      float *v_base, float *v_features,
                                                      float *v_means, float *__restrict__ ws,
                                                      int ws_stride) {
  extern __shared__ __align__(16) float smem[];
  load_head(a.hd, smem);
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = lane & 31, h = lane >> 5;
  float *stage = smem + kLdsHead;
  float *s0 = stage + wave * kLdsWave, *s1 = s0 + kAppWaveRows * kAppSt,
        *sd = s1 + kAppWaveRows * kAppSt;
  float *wrow = ws + (int64_t)blockIdx.x * ws_stride;
  const int64_t ntiles = (a.N + kAppTile - 1) / kAppTile;

  f32x16 dW1[2][2], dW2[2][2];
#pragma unroll
  for (int m = 0; m < 2; ++m)
#pragma unroll
    for (int n = 0; n < 2; ++n)
#pragma unroll
      for (int r = 0; r < 16; ++r) dW1[m][n][r] = dW2[m][n][r] = 0.f;
  // the sums that no MFMA takes, lane = unit: in double, a handful per pass
  double db1 = 0.0, db2 = 0.0, db3 = 0.0, dW3[3] = {0.0, 0.0, 0.0};

  for (int c = 0; c < a.C; ++c) {
    float demb[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) demb[k] = 0.f;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
      const int64_t row = tile * kAppTile + wave * kAppWaveRows + i;
      AppRow x;
      float dB[kAppBases][3];
      app_load_row<true>(a, c, row, h, x, dB);
      // per-row outputs are summed over cameras by the lane that owns them:
      // written for camera 0, read and added to after it
      float vb[3] = {0.f, 0.f, 0.f}, vm[3] = {0.f, 0.f, 0.f};
      f32x16 dX[2];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int r = 0; r < 16; ++r) dX[t][r] = 0.f;
      if (__any(x.valid)) {
        f32x16 H1[2], H2[2];
        app_trunk(smem, x, i, h, H1, H2);
        float base[3] = {0.f, 0.f, 0.f}, dout[3];
        double col[3];
        if (x.valid) {
          base[0] = a.base[3 * row]; base[1] = a.base[3 * row + 1]; base[2] = a.base[3 * row + 2];
        }
        app_head_out(smem, H2, h, base, col);
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const float v = x.valid ? v_colors[((int64_t)c * a.N + row) * 3 + q] : 0.f;
          dout[q] = (float)((double)v * (col[q] * (1.0 - col[q])));
          vb[q] = dout[q];
        }
        // ---- last layer: dW3 = dout H2^T, db3, dZ2
        wave_lds_sync();
        app_stage(s0, H2, i, h);
        app_stage(s1, H1, i, h);
        if (h == 0) {
#pragma unroll
          for (int q = 0; q < 3; ++q) sd[q * kAppWaveRows + i] = dout[q];
        }
        wave_lds_sync();
#pragma unroll 8
        for (int n = 0; n < kAppWaveRows; ++n) {
          const float hv = s0[n * kAppSt + lane];
#pragma unroll
          for (int q = 0; q < 3; ++q) dW3[q] = fma((double)sd[q * kAppWaveRows + n], (double)hv, dW3[q]);
        }
        if (lane < 3) {
#pragma unroll 8
          for (int n = 0; n < kAppWaveRows; ++n) db3 += sd[lane * kAppWaveRows + n];
        }
        f32x16 dZ[2];
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) {
            const int u = acc_unit(r, h, t);
            const float g = (smem[kLdsW3 + u] * dout[0] + smem[kLdsW3 + kAppW + u] * dout[1]) +
                            smem[kLdsW3 + 2 * kAppW + u] * dout[2];
            dZ[t][r] = H2[t][r] > 0.f ? g : 0.f;
          }
        // ---- layer 2: db2, dW2 = dZ2 H1^T, dH1 = W2^T dZ2
        wave_lds_sync();
        app_stage(s0, dZ, i, h);
        wave_lds_sync();
        db2 += app_colsum(s0, lane);
        app_outer(s0, s1, i, h, dW2);
        f32x16 dH[2];
        app_back(smem + kLdsW2, dZ, i, h, dH);
#pragma unroll
        for (int t = 0; t < 2; ++t)
#pragma unroll
          for (int r = 0; r < 16; ++r) dZ[t][r] = H1[t][r] > 0.f ? dH[t][r] : 0.f;
        // ---- layer 1: db1, dW1 = dZ1 X^T, dX = W1^T dZ1
        wave_lds_sync();
        app_stage(s0, dZ, i, h);
        {
          float *xr = s1 + i * kAppSt;
#pragma unroll
          for (int q = 0; q < 2; ++q)
            *reinterpret_cast<float4 *>(xr + 8 * h + 4 * q) =
                make_float4(x.xe[4 * q], x.xe[4 * q + 1], x.xe[4 * q + 2], x.xe[4 * q + 3]);
#pragma unroll
          for (int q = 0; q < 4; ++q)
            *reinterpret_cast<float4 *>(xr + 16 + 16 * h + 4 * q) =
                make_float4(x.xf[4 * q], x.xf[4 * q + 1], x.xf[4 * q + 2], x.xf[4 * q + 3]);
#pragma unroll
          for (int q = 0; q < 2; ++q)
            *reinterpret_cast<float4 *>(xr + 48 + 8 * h + 4 * q) =
                make_float4(x.xb[4 * q], x.xb[4 * q + 1], x.xb[4 * q + 2], x.xb[4 * q + 3]);
        }
        wave_lds_sync();
        db1 += app_colsum(s0, lane);
        app_outer(s0, s1, i, h, dW1);
        app_back(smem + kLdsW1, dZ, i, h, dX);
        // inputs 0..15 are the embedding: tile 0, registers 0..7
#pragma unroll
        for (int k = 0; k < 8; ++k) demb[k] += dX[0][k];
        // inputs 48..63 are the bases: tile 1, registers 8..15 hold basis
        // (r&3) + 8 ((r>>2) - 2) + 4 h; through the basis and the normalisation
        // (a projection that cancels the radial part: summed and projected in
        // double, 27 operations per row)
        double vd[3] = {0.0, 0.0, 0.0};
#pragma unroll
        for (int r = 8; r < 16; ++r) {
          const int b0 = (r & 3) + 8 * ((r >> 2) - 2);
          const double g = (double)dX[1][r];
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            const float lo = b0 < a.nb ? dB[b0][q] : 0.f, hi = b0 + 4 < a.nb ? dB[b0 + 4][q] : 0.f;
            vd[q] = fma(g, (double)(h ? hi : lo), vd[q]);
          }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) {
          const double other = __shfl_xor(vd[q], 32, kWave);
          vd[q] = h ? other + vd[q] : vd[q] + other;
        }
        if (x.valid && x.len > kAppNormEps) {
          const double d0 = x.dir[0], d1 = x.dir[1], d2 = x.dir[2];
          const double dt = d0 * vd[0] + d1 * vd[1] + d2 * vd[2];
          const double inv = 1.0 / (double)x.len;
          vm[0] = (float)((vd[0] - dt * d0) * inv);
          vm[1] = (float)((vd[1] - dt * d1) * inv);
          vm[2] = (float)((vd[2] - dt * d2) * inv);
        }
      }
      if (row < a.N) {
        // features 4h + {0, 8}: tile 0 registers 8..15; 16 + 4h + {0, 8}: tile 1 registers 0..7
        float4 *vf = reinterpret_cast<float4 *>(v_features + row * kAppFeat + 4 * h);
        float4 g[4] = {make_float4(dX[0][8], dX[0][9], dX[0][10], dX[0][11]),
                       make_float4(dX[0][12], dX[0][13], dX[0][14], dX[0][15]),
                       make_float4(dX[1][0], dX[1][1], dX[1][2], dX[1][3]),
                       make_float4(dX[1][4], dX[1][5], dX[1][6], dX[1][7])};
#pragma unroll
        for (int q = 0; q < 4; ++q) {
          if (c > 0) {
            const float4 p = vf[2 * q];
            g[q].x += p.x; g[q].y += p.y; g[q].z += p.z; g[q].w += p.w;
          }
          vf[2 * q] = g[q];
        }
        if (h == 0) {
#pragma unroll
          for (int q = 0; q < 3; ++q) {
            v_base[3 * row + q] = c > 0 ? v_base[3 * row + q] + vb[q] : vb[q];
            v_means[3 * row + q] = c > 0 ? v_means[3 * row + q] + vm[q] : vm[q];
          }
        }
      }
    }
    // the camera's embedding gradient: over the 32 lanes of each half, then
    // over the waves (lane half h holds inputs {0..3, 8..11} + 4 h)
#pragma unroll
    for (int k = 0; k < 8; ++k)
#pragma unroll
      for (int m = 16; m >= 1; m >>= 1) demb[k] += __shfl_xor(demb[k], m, kWave);
    __syncthreads();
    if (i == 0) {
#pragma unroll
      for (int k = 0; k < 8; ++k) stage[wave * kLdsWave + (k & 3) + 8 * (k >> 2) + 4 * h] = demb[k];
    }
    __syncthreads();
    if (threadIdx.x < kAppEmbed)
      wrow[kAppHead + kAppEmbed * c + threadIdx.x] =
          ((stage[threadIdx.x] + stage[kLdsWave + threadIdx.x]) +
           stage[2 * kLdsWave + threadIdx.x]) + stage[3 * kLdsWave + threadIdx.x];
    __syncthreads();  // before any wave stages the next camera's tiles
  }
  app_reduce_tiles(stage, dW1, wave, i, h, wrow + kOffW1);
  app_reduce_tiles(stage, dW2, wave, i, h, wrow + kOffW2);
  app_reduce_lanes(stage, db1, kAppW, wave, lane, wrow + kOffB1);
  app_reduce_lanes(stage, db2, kAppW, wave, lane, wrow + kOffB2);
#pragma unroll
  for (int q = 0; q < 3; ++q) app_reduce_lanes(stage, dW3[q], kAppW, wave, lane, wrow + kOffW3 + q * kAppW);
  app_reduce_lanes(stage, db3, 3, wave, lane, wrow + kOffB3);
}

// column j of the workspace, rows in order
__global__ void __launch_bounds__(256) app_reduce_kernel(const float *__restrict__ ws, int rows,
                                                         int stride, float *__restrict__ grads) {
  const int j = blockIdx.x * 256 + threadIdx.x;
  if (j >= stride) return;
  double s = 0.0;  // at most 256 terms: the sum itself adds no fp32 rounding
#pragma unroll 8
  for (int r = 0; r < rows; ++r) s += (double)ws[(int64_t)r * stride + j];
  grads[j] = (float)s;
}

struct AppAdam {
  float *p[6];  // W1, b1, W2, b2, W3, b3
  float *m, *v;  // [8515], the flat order
  const float *grads;  // [8515 + 16 C]
  float *embeds, *em, *ev;  // [n_images, 16] or null
  const int64_t *embed_ids;
  int n_images, C;
  float ss_head, ss_embed, ib;
  const float *hyper;   // device (ss_head, ib, ss_embed, ib) of a captured step, or null
  const int32_t *skip;  // device flag: non-zero = void step
  float b1, b2, eps, wd;
};

__global__ void __launch_bounds__(256) app_adam_kernel(AppAdam a) {
  if (a.skip && *a.skip) return;
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const float ssh = a.hyper ? a.hyper[0] : a.ss_head, ib = a.hyper ? a.hyper[1] : a.ib;
  const float sse = a.hyper ? a.hyper[2] : a.ss_embed;
  if (e < kAppHead) {
    const int j = (int)e;
    float *p = j < kOffB1   ? a.p[0] + j
               : j < kOffW2 ? a.p[1] + (j - kOffB1)
               : j < kOffB2 ? a.p[2] + (j - kOffW2)
               : j < kOffW3 ? a.p[3] + (j - kOffB2)
               : j < kOffB3 ? a.p[4] + (j - kOffW3)
                            : a.p[5] + (j - kOffB3);
    float w = *p, m = a.m[j], v = a.v[j];
    adam_update(w, a.grads[j], m, v, a.b1, a.b2, a.eps, ssh, ib);
    *p = w;
    a.m[j] = m;
    a.v[j] = v;
    return;
  }
  const int64_t t = e - kAppHead;
  if (!a.embeds || t >= (int64_t)a.n_images * kAppEmbed) return;
  const int64_t row = t / kAppEmbed;
  const int k = (int)(t - row * kAppEmbed);
  float g = 0.f;  // every camera of the step that shows this image, in order
  for (int c = 0; c < a.C; ++c) {
    const int64_t id = a.embed_ids[c];
    const int64_t r = id < 0 ? 0 : (id >= a.n_images ? (int64_t)a.n_images - 1 : id);
    if (r == row) g += a.grads[kAppHead + kAppEmbed * c + k];
  }
  float w = a.embeds[t], m = a.em[t], v = a.ev[t];
  // torch.optim.Adam(weight_decay): g += wd * w, for every row
  g = __fmaf_rn(a.wd, w, g);
  adam_update(w, g, m, v, a.b1, a.b2, a.eps, sse, ib);
  a.embeds[t] = w;
  a.em[t] = m;
  a.ev[t] = v;
}

static int64_t app_grid(int64_t N) {
  const int64_t tiles = (N + kAppTile - 1) / kAppTile;
  return tiles < 1 ? 1 : (tiles > kAppMaxGrid ? kAppMaxGrid : tiles);
}

static int app_check(const char *who, int C, int64_t N, int sh_degree, const float *means,
                     const float *campos, const float *features, const float *base,
                     const float *embeds, const int64_t *embed_ids, int n_images,
                     const float *const *head) {
  GS_REQUIRE(C >= 1 && N >= 0, "%s: C=%d N=%lld", who, C, (long long)N);
  GS_REQUIRE(sh_degree >= 0 && sh_degree <= 3, "%s: sh_degree=%d not in 0..3", who, sh_degree);
  GS_REQUIRE(means && campos && features && base, "%s: null pointer argument", who);
  GS_REQUIRE(head, "%s: null head", who);
  for (int k = 0; k < 6; ++k) GS_REQUIRE(head[k], "%s: null head tensor %d", who, k);
  GS_REQUIRE(!(embeds && embed_ids) || n_images >= 1, "%s: n_images=%d", who, n_images);
  return 0;
}

static AppIn app_in(int C, int64_t N, int sh_degree, const float *means, const float *campos,
                    const float *features, const float *base, const float *embeds,
                    const int64_t *embed_ids, int n_images, const float *const *head,
                    const uint8_t *masks, const int32_t *radii) {
  AppIn a{};
  a.C = C;
  a.N = N;
  a.nb = (sh_degree + 1) * (sh_degree + 1);
  a.means = means;
  a.campos = campos;
  a.features = features;
  a.base = base;
  a.embeds = embeds;
  a.embed_ids = embed_ids;
  a.n_images = n_images;
  a.hd = AppHead{head[0], head[1], head[2], head[3], head[4], head[5]};
  a.masks = masks;
  a.radii = radii;
  return a;
}

}  // namespace gs

using namespace gs;

extern "C" int64_t gsplat_hip_app_workspace_bytes(int64_t N, int C) {
  return app_grid(N) * (kAppHead + kAppEmbed * (int64_t)(C > 0 ? C : 1)) * (int64_t)sizeof(float);
}

extern "C" int gsplat_hip_app_colors_fwd(int C, int64_t N, int sh_degree, const float *means,
                                         const float *campos, const float *features,
                                         const float *base_colors, const float *embeds,
                                         const int64_t *embed_ids, int n_images,
                                         const float *const *head, const uint8_t *masks,
                                         const int32_t *radii, float *colors, void *stream) {
  if (int rc = app_check("app_colors_fwd", C, N, sh_degree, means, campos, features, base_colors,
                         embeds, embed_ids, n_images, head))
    return rc;
  if (N == 0) return 0;
  GS_REQUIRE(colors, "app_colors_fwd: null colors");
  const AppIn a = app_in(C, N, sh_degree, means, campos, features, base_colors, embeds, embed_ids,
                         n_images, head, masks, radii);
  const size_t lds = kLdsHead * sizeof(float);
  hipLaunchKernelGGL(app_fwd_kernel, dim3((unsigned)app_grid(N)), dim3(256), lds,
                     (hipStream_t)stream, a, colors);
  GS_CHECK_LAUNCH("app_colors_fwd");
  return 0;
}

extern "C" int gsplat_hip_app_colors_bwd(int C, int64_t N, int sh_degree, const float *means,
                                         const float *campos, const float *features,
                                         const float *base_colors, const float *embeds,
                                         const int64_t *embed_ids, int n_images,
                                         const float *const *head, const uint8_t *masks,
                                         const int32_t *radii, const float *v_colors,
                                         float *v_base_colors, float *v_features, float *v_means,
                                         void *workspace, void *stream) {
  if (int rc = app_check("app_colors_bwd", C, N, sh_degree, means, campos, features, base_colors,
                         embeds, embed_ids, n_images, head))
    return rc;
  GS_REQUIRE(workspace, "app_colors_bwd: null workspace");
  GS_REQUIRE(N == 0 || (v_colors && v_base_colors && v_features && v_means),
             "app_colors_bwd: null pointer argument");
  const AppIn a = app_in(C, N, sh_degree, means, campos, features, base_colors, embeds, embed_ids,
                         n_images, head, masks, radii);
  const size_t lds = (kLdsHead + 4 * kLdsWave) * sizeof(float);
  // more than the 64 KiB a kernel gets by default: raised once per device, at
  // the first launch there (not again on later launches, so a launch inside
  // a stream capture -- which a warm-up step precedes -- makes no such call)
  static std::atomic<uint64_t> lds_raised{0};
  int dev = 0;
  GS_HIP(hipGetDevice(&dev));
  const uint64_t bit = 1ull << (dev & 63);
  if (!(lds_raised.load(std::memory_order_acquire) & bit)) {
    GS_HIP(hipFuncSetAttribute(reinterpret_cast<const void *>(app_bwd_kernel),
                               hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    lds_raised.fetch_or(bit, std::memory_order_release);
  }
  // N == 0 still writes the (single, zero) workspace row
  hipLaunchKernelGGL(app_bwd_kernel, dim3((unsigned)app_grid(N)), dim3(256), lds,
                     (hipStream_t)stream, a, v_colors, v_base_colors, v_features, v_means,
                     reinterpret_cast<float *>(workspace), kAppHead + kAppEmbed * C);
  GS_CHECK_LAUNCH("app_colors_bwd");
  return 0;
}

extern "C" int gsplat_hip_app_reduce_adam(int C, int64_t N, const void *workspace, float *grads,
                                          int apply, float *const *head, float *head_exp_avg,
                                          float *head_exp_avg_sq, float *embeds,
                                          const int64_t *embed_ids, int n_images,
                                          float *embed_exp_avg, float *embed_exp_avg_sq, float lr,
                                          float beta1, float beta2, float eps,
                                          float embed_lr_mult, float embed_weight_decay, int step,
                                          const float *hyper_device, const int32_t *skip_device,
                                          void *stream) {
  GS_REQUIRE(C >= 1 && N >= 0, "app_reduce_adam: C=%d N=%lld", C, (long long)N);
  GS_REQUIRE(workspace && grads, "app_reduce_adam: null workspace or grads");
  const int stride = kAppHead + kAppEmbed * C;
  hipLaunchKernelGGL(app_reduce_kernel, dim3((stride + 255) / 256), dim3(256), 0,
                     (hipStream_t)stream, reinterpret_cast<const float *>(workspace),
                     (int)app_grid(N), stride, grads);
  GS_CHECK_LAUNCH("app_reduce_adam (reduce)");
  if (!apply) return 0;
  GS_REQUIRE(head && head_exp_avg && head_exp_avg_sq, "app_reduce_adam: null head state");
  for (int k = 0; k < 6; ++k) GS_REQUIRE(head[k], "app_reduce_adam: null head tensor %d", k);
  GS_REQUIRE(!embeds || (embed_ids && embed_exp_avg && embed_exp_avg_sq && n_images >= 1),
             "app_reduce_adam: embeds without ids, moments or n_images");
  GS_REQUIRE(hyper_device || step >= 1, "app_reduce_adam: step >= 1, or hyper");
  AppAdam a{};
  for (int k = 0; k < 6; ++k) a.p[k] = head[k];
  a.m = head_exp_avg;
  a.v = head_exp_avg_sq;
  a.grads = grads;
  a.embeds = embeds;
  a.em = embed_exp_avg;
  a.ev = embed_exp_avg_sq;
  a.embed_ids = embed_ids;
  a.n_images = n_images;
  a.C = C;
  a.hyper = hyper_device;
  a.skip = skip_device;
  a.b1 = beta1;
  a.b2 = beta2;
  a.eps = eps;
  a.wd = embed_weight_decay;
  if (!hyper_device) {  // gsplat_hip_adam_step's host arithmetic
    const double bc1 = 1.0 - pow((double)beta1, step), bc2 = 1.0 - pow((double)beta2, step);
    a.ss_head = (float)(lr / bc1);
    a.ss_embed = (float)((double)lr * embed_lr_mult / bc1);
    a.ib = (float)(1.0 / sqrt(bc2));
  }
  const int64_t total = kAppHead + (embeds ? (int64_t)n_images * kAppEmbed : 0);
  hipLaunchKernelGGL(app_adam_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0,
                     (hipStream_t)stream, a);
  GS_CHECK_LAUNCH("app_reduce_adam (adam)");
  return 0;
}
