// The body of ssim::fused_kernel (GS_FUSED_MASKED 0) and of
// ssim::fused_masked_kernel (GS_FUSED_MASKED 1), included by ssim.hip inside
// each of the two (their parameters and the template constants C, BR, CPW,
// XS are the names used here).  Text, not a shared device function or a
// template flag: the plain kernel is then the same tokens as before the
// masked one existed and compiles to the same device code
// (tools/kernel_isa_diff.py) -- as an inlined function with the flag it did not.
//
// Masked: the render is composed before the loss, per pixel
//   x = (mask ? render : 0) + bkgd[c] * (1 - alpha)
// (simple_trainer.py:505-506, 629-631).  mask: uint8 [B,H,W], or a stack
// indexed by y_index like y; null: all valid.  alpha [B,H,W] and bkgd [B,C]
// are read only where bkgd is non-null.  The window's mask is one bit per
// loaded row in a register, its 1 - alpha sits in LDS (each thread re-reads
// what it wrote); s_xy then holds the composed x, so the statistics and the
// L1 are the plain kernel's; the own pixels are composed again from global
// memory before pass C2 instead of being held over pass A.  grad = mask ? u : 0
// with u = dL/dx, and grad_alpha = -sum_c bkgd[c] u_c accumulates over the
// channel loop in two LDS slots of the thread that writes the pixel's grad
// (all channels of a tile run in one workgroup; as registers the two sums
// were live over pass B and spilled): no atomics, no second pass, no
// cross-workgroup reduction, the same bits every run.
  static_assert(C % CPW == 0, "channel groups");
  constexpr int CG = C / CPW;
  __shared__ __attribute__((aligned(16))) char lds[kFusedLds];
  __shared__ float red[2][kFThreads / 64];
#if GS_FUSED_MASKED
  // 1 - alpha of the window, written and read back by the same thread (the
  // lane / row mapping of load and stage): no barrier of its own
  __shared__ float s_wa[FI][FI];
  // the alpha gradient of each thread's two own pixels, summed over the
  // channel loop in slots of its own (as registers they were pass B's)
  __shared__ float s_ga[2][kFThreads];
#endif
  f2v(*s_xy)[SX] = reinterpret_cast<f2v(*)[SX]>(lds);
  f2v(*hA)[SH] = reinterpret_cast<f2v(*)[SH]>(lds + kOffA);
  f2v(*hB)[SH] = reinterpret_cast<f2v(*)[SH]>(lds + kOffB);
  float(*hC)[SH] = reinterpret_cast<float(*)[SH]>(lds + kOffC);
  f2v(*m01)[SH] = reinterpret_cast<f2v(*)[SH]>(lds);
  float(*m2)[SH] = reinterpret_cast<float(*)[SH]>(lds + FM * SH * 8);
  f2v(*g01)[SG] = reinterpret_cast<f2v(*)[SG]>(lds + kOffA);
  float(*g2)[SG] = reinterpret_cast<float(*)[SG]>(lds + kOffA + FM * SG * 8);

  const int Hm = H - 2 * R, Wm = W - 2 * R;
  const int tx = (W + FT - 1) / FT, ty = (H + FT - 1) / FT, nt = tx * ty, ntc = nt * CG;
  // XCD-aware: workgroup L runs on XCD L % 8; each XCD takes a contiguous
  // run of (tile, channel group)s so neighbouring windows' shared apron rows
  // (and a tile's other channel groups) hit its L2
  const int per = (ntc + 7) / 8, L = blockIdx.x;
  const int b = L / (8 * per), q = L - b * 8 * per;
  const int tc = (q & 7) * per + (q >> 3);
  if (b >= B || tc >= ntc) return;
  const int t = tc / CG, cg = tc - t * CG;
  if (y_index) y += y_index[0] * ((int64_t)B * H * W * C);  // image y_index of a stack
  const int qi0 = (t / tx) * FT, qj0 = (t % tx) * FT;  // image tile origin
  const int ri0 = qi0 - 2 * R, rj0 = qj0 - 2 * R;       // window origin (image coords)
  const int tid = threadIdx.x, lane = tid & 63;
  const int w8 = __builtin_amdgcn_readfirstlane(tid >> 6);

  // window loads of one channel: lane = window column, wave w = rows w, w+8,
  // ...; clamped addresses (unconditional loads), zeroed outside the image
  // (row pointers are wave-uniform: saddr + one 32-bit lane offset per load)
  // x (the render, and its gradient) has XS >= C floats per pixel (an RGB+D
  // render read in place: XS = 4, C = 3); y has C
  const int colc = min(max(rj0 + lane, 0), W - 1);
  const uint32_t lox = (uint32_t)(colc * XS), loy = (uint32_t)(colc * C);
  const bool col_ok = lane < FI && rj0 + lane >= 0 && rj0 + lane < W;
  const float *xb = x + (int64_t)b * H * W * XS, *yb = y + (int64_t)b * H * W * C;
  float vx[kFRows], vy[kFRows];
  auto load = [&](int c) {
#pragma unroll
    for (int k = 0; k < kFRows; ++k) {
      const int64_t row = (int64_t)min(max(ri0 + w8 + 8 * k, 0), H - 1) * W;
      vx[k] = (xb + row * XS)[lox + c];
      vy[k] = (yb + row * C)[loy + c];
    }
  };
  float lsum = 0.f, ssum = 0.f;
#if GS_FUSED_MASKED
  // bit k of wm: the mask at window row w8 + 8 k of this lane's column; bits
  // 16, 17: at the thread's two own pixels (image rows 2 gr, 2 gr + 1, column
  // gc)
  uint32_t wm = ~0u;
  s_ga[0][tid] = 0.f;
  s_ga[1][tid] = 0.f;
  // own pixel j's index in its image, clamped, from the thread index t_.
  // The channel loop forms it from an opaque copy of tid each time round:
  // hoisted out of the loop, the pixels' 64-bit addresses were live over
  // passes A and B and spilled
  auto own = [&](int t_, int j) {
    return (uint32_t)(min(qi0 + 2 * (t_ >> 5) + j, H - 1) * W + min(qj0 + (t_ & 31), W - 1));
  };
  float *gb = grad + (int64_t)b * H * W * XS;
  if (mask) {
    if (y_index) mask += y_index[0] * ((int64_t)B * H * W);
    const uint8_t *mb = mask + (int64_t)b * H * W;
    wm = 0u;
#pragma unroll
    for (int k = 0; k < kFRows; ++k) {
      const int64_t row = (int64_t)min(max(ri0 + w8 + 8 * k, 0), H - 1) * W;
      wm |= (mb + row)[colc] ? (1u << k) : 0u;
    }
#pragma unroll
    for (int j = 0; j < 2; ++j) wm |= mb[own(tid, j)] ? (0x10000u << j) : 0u;
  }
  const float *bk = bkgd ? bkgd + b * C : nullptr;
  if (bk) {
    const float *ab = alpha + (int64_t)b * H * W;
#pragma unroll
    for (int k = 0; k < kFRows; ++k) {
      const int r = w8 + 8 * k;
      const int64_t row = (int64_t)min(max(ri0 + r, 0), H - 1) * W;
      if (r < FI && lane < FI) s_wa[r][lane] = 1.f - (ab + row)[colc];
    }
  }
#endif
  // backward vertical pass mapping: column gc, image rows 2 gr, 2 gr + 1
  const int gc = tid & 31, gr = tid >> 5;
  // the loaded window into s_xy (+ its L1 over the tile's own pixels, window
  // rows / cols 2R .. 2R+31)
#if GS_FUSED_MASKED
  // x = (mask ? render : 0) + bkgd[c] (1 - alpha): a select, so a non-finite
  // render value under the mask is gone
  auto stage = [&](int c) {
    const float bc = bk ? bk[c] : 0.f;
#pragma unroll
    for (int k = 0; k < kFRows; ++k) {
      const int r = w8 + 8 * k, gi = ri0 + r;
      const bool ok = col_ok && r < FI && gi >= 0 && gi < H;
      float a = ok && ((wm >> k) & 1u) ? vx[k] : 0.f;
      const float bb = ok ? vy[k] : 0.f;
      if (bk && ok) a += bc * s_wa[r][lane];
#else
  auto stage = [&](int) {
#pragma unroll
    for (int k = 0; k < kFRows; ++k) {
      const int r = w8 + 8 * k, gi = ri0 + r;
      const bool ok = col_ok && r < FI && gi >= 0 && gi < H;
      const float a = ok ? vx[k] : 0.f, bb = ok ? vy[k] : 0.f;
#endif
      if (r < FI && lane < FI) s_xy[r][lane] = f2v{a, bb};
      if (r >= 2 * R && r < 2 * R + FT && lane >= 2 * R && lane < 2 * R + FT)
        lsum += fabsf(a - bb);
    }
  };
  // The next channel's window is loaded while pass C1 runs (its latency
  // hidden behind C1) and staged while C2 runs: s_xy's last readers of this
  // channel (pass C1, through m01 / m2) are behind C1's barrier, and this
  // channel's own pixels (px0 / px1) were read into registers before pass A.
  const int c_end = cg * CPW + CPW;
  load(cg * CPW);
  stage(cg * CPW);
  __syncthreads();
#pragma nounroll
  for (int c = cg * CPW; c < c_end; ++c) {
#if !GS_FUSED_MASKED
    const f2v px0 = s_xy[2 * R + 2 * gr][2 * R + gc], px1 = s_xy[2 * R + 2 * gr + 1][2 * R + gc];
#endif
    // ---- A: horizontal blur of the statistics, FI rows x FM columns
    static_assert(FM % kHA == 0 && FT % kHC == 0, "pass A / C1 blocking");
    for (int idx = tid; idx < FI * (FM / kHA); idx += kFThreads) {
      const int jg = idx / FI, r = idx - jg * FI, j0 = jg * kHA;
      f2v v[K + kHA - 1], sq[K + kHA - 1];
      float xy[K + kHA - 1];
#pragma unroll
      for (int i = 0; i < K + kHA - 1; ++i) {
        v[i] = s_xy[r][j0 + i];
        sq[i] = v[i] * v[i];
        xy[i] = v[i].x * v[i].y;
      }
#pragma unroll
      for (int o = 0; o < kHA; ++o) {
        f2v a = {0.f, 0.f}, bb = {0.f, 0.f};
        float cc = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float g = kG[k];
          a = __builtin_elementwise_fma(f2v{g, g}, v[o + k], a);
          bb = __builtin_elementwise_fma(f2v{g, g}, sq[o + k], bb);
          cc = __builtin_fmaf(g, xy[o + k], cc);
        }
        hA[r][j0 + o] = a;
        hB[r][j0 + o] = bb;
        hC[r][j0 + o] = cc;
      }
    }
    __syncthreads();
    // ---- B: vertical blur -> the partials of map pixels (local rows / cols
    // 0..FM-1 = map coords ri0.., rj0..; zero outside the valid map), into s_xy
    constexpr int kItems = (FM + BR - 1) / BR * FM;
    for (int it = tid; it < kItems; it += kFThreads) {
      const int mg = it / FM, mc = it - mg * FM;
      f2v oa[BR], ob[BR];
      float oc[BR];
#pragma unroll
      for (int j = 0; j < BR; ++j) {
        oa[j] = f2v{0.f, 0.f};
        ob[j] = f2v{0.f, 0.f};
        oc[j] = 0.f;
      }
#pragma unroll
      for (int i = 0; i < K + BR - 1; ++i) {
        const int r = min(BR * mg + i, FI - 1);  // rows past FI only feed discarded outputs
        const f2v a = hA[r][mc], bb = hB[r][mc];
        const float cc = hC[r][mc];
#pragma unroll
        for (int j = 0; j < BR; ++j) {
          const int k = i - j;
          if (k >= 0 && k < K) {
            const float g = kG[k];
            oa[j] = __builtin_elementwise_fma(f2v{g, g}, a, oa[j]);
            ob[j] = __builtin_elementwise_fma(f2v{g, g}, bb, ob[j]);
            oc[j] = __builtin_fmaf(g, cc, oc[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < BR; ++j) {
        const int mr = BR * mg + j, pi = ri0 + mr, pj = rj0 + mc;
        float p0 = 0.f, p1 = 0.f, p2 = 0.f;
        if (pi >= 0 && pi < Hm && pj >= 0 && pj < Wm) {
          const float u1 = oa[j].x, u2 = oa[j].y;
          const float s11 = ob[j].x - u1 * u1, s22 = ob[j].y - u2 * u2, s12 = oc[j] - u1 * u2;
          const float A1 = 2.f * u1 * u2 + C1, A2 = 2.f * s12 + C2;
          const float B1 = u1 * u1 + u2 * u2 + C1, B2 = s11 + s22 + C2;
          const float inv = 1.f / (B1 * B2);
          const float sv = A1 * A2 * inv;
          if (mr >= 2 * R && mr < FM && mc >= 2 * R) ssum += sv;  // the tile's own map pixels
          const float dN = 2.f * u2 * (A2 - A1), dD = 2.f * u1 * (B2 - B1);
          p0 = (dN - sv * dD) * inv;
          p1 = -sv * B1 * inv;
          p2 = 2.f * A1 * inv;
        }
        if (mr < FM) {
          m01[mr][mc] = f2v{p0, p1};
          m2[mr][mc] = p2;
        }
      }
    }
    __syncthreads();
    const bool more = c + 1 < c_end;
    if (more) load(c + 1);
#if GS_FUSED_MASKED
    // the own pixels' render, target and 1 - alpha again from global memory
    // (clamped addresses; in flight behind pass C1 like the next window):
    // held in registers from before pass A, as px0 / px1 are, they spilled
    float ox[2], oy[2], ow[2];
    int tq = tid;
    asm volatile("" : "+v"(tq));
    const uint32_t po[2] = {own(tq, 0), own(tq, 1)};
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      ox[j] = xb[po[j] * XS + c];
      oy[j] = yb[po[j] * C + c];
      ow[j] = bk ? 1.f - (alpha + (int64_t)b * H * W)[po[j]] : 0.f;
    }
#endif
    // ---- C1: horizontal blur of the partials, FM rows x FT columns (the
    // adjoint of the valid correlation: full correlation with the symmetric
    // kernel, see bwd_kernel), into hA
    for (int idx = tid; idx < FM * (FT / kHC); idx += kFThreads) {
      const int jg = idx / FM, r = idx - jg * FM, j0 = jg * kHC;
      f2v v[K + kHC - 1];
      float w[K + kHC - 1];
#pragma unroll
      for (int i = 0; i < K + kHC - 1; ++i) {
        v[i] = m01[r][j0 + i];
        w[i] = m2[r][j0 + i];
      }
#pragma unroll
      for (int o = 0; o < kHC; ++o) {
        f2v a = {0.f, 0.f};
        float cc = 0.f;
#pragma unroll
        for (int k = 0; k < K; ++k) {
          const float g = kG[k];
          a = __builtin_elementwise_fma(f2v{g, g}, v[o + k], a);
          cc = __builtin_fmaf(g, w[o + k], cc);
        }
        g01[r][j0 + o] = a;
        g2[r][j0 + o] = cc;
      }
    }
    __syncthreads();
    if (more) stage(c + 1);  // the next channel's window (s_xy is free: see above)
    // ---- C2: vertical blur onto the tile pixels, gradient out.  (The next
    // channel's pass A rewrites hA, which C2 reads, only after the barrier
    // below.)
    {
      f2v oa[2] = {f2v{0.f, 0.f}, f2v{0.f, 0.f}};
      float oc[2] = {0.f, 0.f};
#pragma unroll
      for (int i = 0; i < K + 1; ++i) {
        const int r = 2 * gr + i;
        const f2v a = g01[r][gc];
        const float cc = g2[r][gc];
#pragma unroll
        for (int j = 0; j < 2; ++j) {
          const int k = i - j;
          if (k >= 0 && k < K) {
            const float g = kG[k];
            oa[j] = __builtin_elementwise_fma(f2v{g, g}, a, oa[j]);
            oc[j] = __builtin_fmaf(g, cc, oc[j]);
          }
        }
      }
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        const int qi = qi0 + 2 * gr + j, qj = qj0 + gc;
#if GS_FUSED_MASKED
        f2v v = {(wm >> (16 + j)) & 1u ? ox[j] : 0.f, oy[j]};
        if (bk) v.x += bk[c] * ow[j];
#else
        const f2v v = j ? px1 : px0;
#endif
        const float d = v.x - v.y;
        const float sgn = d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f);
#if GS_FUSED_MASKED
        // u = dL/dx: the colour gradient where the mask lets the render
        // through, and its share of the alpha gradient -sum_c bkgd[c] u_c
        // (with the roundings the compiler gives the plain kernel's
        // expression below -- one fma, for v.y * oc -- spelled out, so that
        // with every pixel valid and no background the two kernels' gradients
        // are the same bits)
        float u;
        {
#pragma clang fp contract(off)
          const float t = oa[j].x + (2.f * v.x) * oa[j].y;
          u = cs * __builtin_fmaf(v.y, oc[j], t) + cl * sgn;
        }
        if (bk) s_ga[j][tid] -= bk[c] * u;
        if (qi < H && qj < W)
          gb[po[j] * XS + c] = (wm >> (16 + j)) & 1u ? u : 0.f;
#else
        if (qi < H && qj < W)
          grad[(((int64_t)b * H + qi) * W + qj) * XS + c] =
              cs * (oa[j].x + 2.f * v.x * oa[j].y + v.y * oc[j]) + cl * sgn;
#endif
      }
    }
    if (more) __syncthreads();  // the staged window, and C2's reads of hA done
  }
  if (XS > C && cg == CG - 1) {  // the render's other channels: no loss term, zero gradient
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int qi = qi0 + 2 * gr + j, qj = qj0 + gc;
      if (qi < H && qj < W)
        for (int e = C; e < XS; ++e) grad[(((int64_t)b * H + qi) * W + qj) * XS + e] = 0.f;
    }
  }
#if GS_FUSED_MASKED
  if (bk) {
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int qi = qi0 + 2 * gr + j, qj = qj0 + gc;
      if (qi < H && qj < W) (grad_alpha + (int64_t)b * H * W)[own(tid, j)] = s_ga[j][tid];
    }
  }
#endif
  ssum = wave_sum(ssum);
  lsum = wave_sum(lsum);
  if (lane == 0) {
    red[0][tid >> 6] = ssum;
    red[1][tid >> 6] = lsum;
  }
  __syncthreads();
  if (tid == 0) {
    float s = 0.f, l = 0.f;
    for (int w = 0; w < kFThreads / 64; ++w) {
      s += red[0][w];
      l += red[1][w];
    }
    partials[2 * ((int64_t)b * ntc + tc)] = s;
    partials[2 * ((int64_t)b * ntc + tc) + 1] = l;
  }
