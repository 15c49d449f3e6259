// window.h — the 3-D sliding window of the validation loops between "volume in HBM" and "label map in HBM"
// (the reference's val_3D.py:18-73: pad, window grid, soft-max, score / count maps, divide, arg-max, crop; :128-132: MONAI's
// sliding_window_inference; restated in icl_amd/val_3D.py) as three HBM-bound streams:
//   window_gather_kernel      F.pad + one slice per window + stack + contiguous      -> [n, Cin, r0, r1, r2], bit-equal
//   window_accumulate_kernel  soft-max (optional) + score[:, window] += value (* importance) + weight[window] += 1 (importance)
//   window_finalize_kernel    score / weight, arg-max over the classes, crop          -> int64 labels (+ the cropped quotients)
// The last volume axis is the fastest one; 16-byte accesses per lane where the alignment allows (V = 4), a scalar form otherwise
// (V = 1); grid-stride launches; no LDS, no atomics.  In the accumulation ONE thread owns a destination voxel (or a quad of them) and
// walks the batch's windows in their given order, so overlapping windows of one batch neither race nor change the order of the adds:
// every sum is the one the torch loop forms, window by window.
// Mirror test-time augmentation: the instantiations window_gather_kernel<V, WinFlips> and window_accumulate_kernel<NCMAX, V, WinFlips>
// take one mask per window of the batch behind their other arguments (a "pass": bit a set = axis a of the window mirrored).  The gather
// writes flip(window, axes) — the same gather with a reversed source index; the accumulate adds flip(value, axes) — the same
// read-modify-write with a reversed read of the logits, the importance map staying in the volume's frame.  Without the trailing
// argument (FL empty) nothing of the masks is compiled in: the plain instantiations are the kernels they were.
#pragma once

namespace icl {

constexpr int kWinMaxBatch = 16;
constexpr int kWinMaxClasses = 256;

struct WinBatch {
  int o[kWinMaxBatch][3];      // window origins in the PADDED frame
};
struct WinExt {
  int d0, d1, d2;
};
// one mirror mask per window of the batch, bit a set = axis a mirrored (0 .. 7): window w's mask in bits 4 w .. 4 w + 2.  One 64-bit
// kernel argument on purpose: it arrives with one scalar load and a mask is a scalar shift (a byte array indexed by the pass was a
// VECTOR byte load and a wait in front of every pass's loads — measured at 7 to 9 % of a launch).
struct WinFlips {
  unsigned long long m;
};
static_assert(kWinMaxBatch * 4 <= 64, "four bits per window in WinFlips::m");

// product and sum of the weighted accumulation, each rounded on its own (the torch loop forms `w * value`, then adds).  hipcc contracts
// a * b + c into an fma by default — also through __fmul_rn / __fadd_rn, which are plain operators in its headers — so both are
// formed here with contraction off.  The pragma is clang's: the CPU emulator build (g++, tests/hipemu) keeps the two roundings because it
// targets baseline x86-64, which has no fused multiply-add to contract into; an emulator build with -mfma / -march=native would need
// -ffp-contract=off as well (tests/test_window_emu.py's equality with the torch loop in the Gaussian logits form would show it).
__device__ __forceinline__ float win_mul(float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a * b;
}
__device__ __forceinline__ float win_add(float a, float b) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  return a + b;
}

template <int V>
__device__ __forceinline__ void win_load(const float* __restrict__ p, float* v) {
  if constexpr (V == 4) {
    const float4 q = *reinterpret_cast<const float4*>(p);
    v[0] = q.x; v[1] = q.y; v[2] = q.z; v[3] = q.w;
  } else {
    v[0] = p[0];
  }
}
template <int V>
__device__ __forceinline__ void win_store(float* __restrict__ p, const float* v) {
  if constexpr (V == 4) {
    *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
  } else {
    p[0] = v[0];
  }
}

__device__ __forceinline__ int win_mask(int) { return 0; }
__device__ __forceinline__ int win_mask(int w, const WinFlips& fl) { return (int)(fl.m >> (4 * w)) & 7; }

// a window's values along a mirrored last axis: the quad's lanes reversed when `rev` (a single value has no order); nothing without FLIP
template <int V, bool FLIP>
__device__ __forceinline__ void win_reverse(float* v, int rev) {
  if constexpr (FLIP && V == 4) {
    if (rev) {
      const float t0 = v[0], t1 = v[1];
      v[0] = v[3]; v[1] = v[2]; v[2] = t1; v[3] = t0;
    }
  }
}
template <int V, bool FLIP>
__device__ __forceinline__ void win_load_pass(const float* __restrict__ p, float* v, int rev) {
  win_load<V>(p, v);
  win_reverse<V, FLIP>(v, rev);
}

// out [n][Cin][r0][r1][r2] <- vol [Cin][s0][s1][s2]; window w (= blockIdx.y) starts at wb.o[w] - a in the unpadded volume, voxels
// outside it read as 0.  V = 4: r2 % 4 == 0 and 16-byte aligned pointers (the store is always a quad; the load is one where the quad
// lies inside the row at a 16-byte aligned address, four guarded scalar loads otherwise).
// fl (FLIP): window w is written mirrored along the axes of its mask in fl — destination (i, j, l) reads the source of (r0 - 1 - i, j, l) for bit 0,
// likewise bits 1 and 2; with V = 4 and bit 2 the destination quad l .. l + 3 is the source quad at r2 - 4 - l with its lanes reversed,
// loaded under the same condition (the zero fill is the unflipped window's, mirrored with it).
template <int V, typename... FL>
__global__ __launch_bounds__(256) void window_gather_kernel(const float* __restrict__ vol, float* __restrict__ out, WinBatch wb, int cin, WinExt s,
                                                            WinExt a, WinExt r, FL... fl) {
  constexpr bool FLIP = sizeof...(FL) > 0;
  const int w = blockIdx.y;
  const int f = win_mask(w, fl...);
  const int b0 = wb.o[w][0] - a.d0, b1 = wb.o[w][1] - a.d1, b2 = wb.o[w][2] - a.d2;
  const int r2v = r.d2 / V;
  const long total = (long)cin * r.d0 * r.d1 * r2v;
  float* __restrict__ dst = out + (long)w * total * V;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    long t = e;
    const int l = (int)(t % r2v) * V;
    t /= r2v;
    const int j = (int)(t % r.d1);
    t /= r.d1;
    const int i = (int)(t % r.d0), ci = (int)(t / r.d0);
    int x = b0 + i, y = b1 + j, z = b2 + l;
    if constexpr (FLIP) {
      if (f & 1) x = b0 + r.d0 - 1 - i;
      if (f & 2) y = b1 + r.d1 - 1 - j;
      if (f & 4) z = b2 + r.d2 - V - l;
    }
    float v[V];
#pragma unroll
    for (int u = 0; u < V; ++u) v[u] = 0.f;
    if (x >= 0 && x < s.d0 && y >= 0 && y < s.d1) {
      const long row = (((long)ci * s.d0 + x) * s.d1 + y) * s.d2;
      if (V == 4 && z >= 0 && z + V <= s.d2 && ((row + z) & 3) == 0) {
        win_load<V>(vol + row + z, v);
      } else {
#pragma unroll
        for (int u = 0; u < V; ++u)
          if (z + u >= 0 && z + u < s.d2) v[u] = vol[row + z + u];
      }
    }
    win_reverse<V, FLIP>(v, f & 4);
    win_store<V>(dst + e * V, v);
  }
}

// score [C][p0][p1][p2] and weight [p0][p1][p2] += the batch's n windows, logits [n][C][r0][r1][r2]; the launch covers the bounding box
// lo .. lo + ext of the windows.  softmax != 0: the value is the soft-max over the class axis of the window's logits (max-subtracted
// expf, sum in class order: softmax_vec of loss.h), else the logits as they are.  imp == nullptr: score += value (no multiply),
// weight += 1; else score = score + imp * value (product and sum rounded separately), weight += imp ([r0][r1][r2]).
// NCMAX = 4 / 16: the classes of a voxel stay in registers (C <= NCMAX).  NCMAX = 0 (16 < C <= 256): nothing indexed by the class is kept;
// per window the class axis is walked for the maximum and for the sum of the soft-max, then once more with the read-modify-write of
// the score map (the logits form takes that last walk only).
// V = 4: p2, r2 and every origin's last coordinate are multiples of 4 and the pointers 16-byte aligned, so a quad lies inside or
// outside a window as a whole.
// fl (FLIP): window w's logits are those of the window mirrored along the axes of its mask in fl; the value added at (dx, dy, dz) of the window is
// the one at the mirrored offset (r0 - 1 - dx for bit 0, likewise bits 1 and 2; V = 4 and bit 2: the quad at r2 - 4 - dz, aligned as r2
// and dz are multiples of 4, lanes reversed).  The importance map is read at (dx, dy, dz): it lives in the volume's frame.
template <int NCMAX, int V, typename... FL>
__global__ __launch_bounds__(256) void window_accumulate_kernel(const float* __restrict__ logits, const float* __restrict__ imp,
                                                                float* __restrict__ score, float* __restrict__ weight, WinBatch wb, int n, int C,
                                                                WinExt p, WinExt r, WinExt lo, WinExt ext, int softmax, FL... fl) {
  constexpr bool FLIP = sizeof...(FL) > 0;
  constexpr int NA = NCMAX > 0 ? NCMAX : 1;
  const int e2v = ext.d2 / V;
  const long total = (long)ext.d0 * ext.d1 * e2v;
  const long P = (long)r.d0 * r.d1 * r.d2, S = (long)p.d0 * p.d1 * p.d2;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    long t = e;
    const int z = lo.d2 + (int)(t % e2v) * V;
    t /= e2v;
    const int y = lo.d1 + (int)(t % ext.d1), x = lo.d0 + (int)(t / ext.d1);
    unsigned hit = 0;
    for (int w = 0; w < n; ++w) {
      const unsigned dx = (unsigned)(x - wb.o[w][0]), dy = (unsigned)(y - wb.o[w][1]), dz = (unsigned)(z - wb.o[w][2]);
      if (dx < (unsigned)r.d0 && dy < (unsigned)r.d1 && dz < (unsigned)r.d2) hit |= 1u << w;
    }
    if (!hit) continue;      // a hole of the bounding box
    const long idx = ((long)x * p.d1 + y) * p.d2 + z;
    float acc[NA][V], wacc[V];
    win_load<V>(weight + idx, wacc);
    if constexpr (NCMAX > 0) {
#pragma unroll
      for (int c = 0; c < NCMAX; ++c) {
#pragma unroll
        for (int u = 0; u < V; ++u) acc[c][u] = 0.f;
        if (c < C) win_load<V>(score + (long)c * S + idx, acc[c]);
      }
    }
    for (int w = 0; w < n; ++w) {
      if (!((hit >> w) & 1u)) continue;
      const long off = ((long)(x - wb.o[w][0]) * r.d1 + (y - wb.o[w][1])) * r.d2 + (z - wb.o[w][2]);
      long offl = off;
      int rev = 0;
      if constexpr (FLIP) {
        const int f = win_mask(w, fl...);
        const int dx = x - wb.o[w][0], dy = y - wb.o[w][1], dz = z - wb.o[w][2];
        rev = f & 4;
        offl = ((long)((f & 1) ? r.d0 - 1 - dx : dx) * r.d1 + ((f & 2) ? r.d1 - 1 - dy : dy)) * r.d2 + (rev ? r.d2 - V - dz : dz);
      }
      const float* __restrict__ lp = logits + (long)w * C * P + offl;
      float wv[V];
#pragma unroll
      for (int u = 0; u < V; ++u) wv[u] = 1.0f;
      if (imp) win_load<V>(imp + off, wv);
#pragma unroll
      for (int u = 0; u < V; ++u) wacc[u] = win_add(wacc[u], wv[u]);
      if constexpr (NCMAX > 0) {
        float val[V][NCMAX];
#pragma unroll
        for (int c = 0; c < NCMAX; ++c) {
          float q[V];
#pragma unroll
          for (int u = 0; u < V; ++u) q[u] = 0.f;
          if (c < C) win_load_pass<V, FLIP>(lp + (long)c * P, q, rev);
#pragma unroll
          for (int u = 0; u < V; ++u) val[u][c] = q[u];
        }
        if (softmax) {
#pragma unroll
          for (int u = 0; u < V; ++u) {
            float lse;
            softmax_vec<NCMAX>(val[u], C, lse);
          }
        }
        if (imp) {
#pragma unroll
          for (int c = 0; c < NCMAX; ++c)
#pragma unroll
            for (int u = 0; u < V; ++u) acc[c][u] = win_add(acc[c][u], win_mul(wv[u], val[u][c]));
        } else {
#pragma unroll
          for (int c = 0; c < NCMAX; ++c)
#pragma unroll
            for (int u = 0; u < V; ++u) acc[c][u] = win_add(acc[c][u], val[u][c]);
        }
      } else {
        float m[V], inv[V];
        if (softmax) {
          win_load_pass<V, FLIP>(lp, m, rev);
          for (int c = 1; c < C; ++c) {
            float q[V];
            win_load_pass<V, FLIP>(lp + (long)c * P, q, rev);
#pragma unroll
            for (int u = 0; u < V; ++u) m[u] = fmaxf(m[u], q[u]);
          }
          float sum[V];
#pragma unroll
          for (int u = 0; u < V; ++u) sum[u] = 0.f;
          for (int c = 0; c < C; ++c) {
            float q[V];
            win_load_pass<V, FLIP>(lp + (long)c * P, q, rev);
#pragma unroll
            for (int u = 0; u < V; ++u) sum[u] += expf(q[u] - m[u]);
          }
#pragma unroll
          for (int u = 0; u < V; ++u) inv[u] = 1.0f / sum[u];
        }
        for (int c = 0; c < C; ++c) {
          float q[V], a[V];
          win_load_pass<V, FLIP>(lp + (long)c * P, q, rev);
          win_load<V>(score + (long)c * S + idx, a);
#pragma unroll
          for (int u = 0; u < V; ++u) {
            if (softmax) q[u] = win_mul(expf(q[u] - m[u]), inv[u]);
            a[u] = imp ? win_add(a[u], win_mul(wv[u], q[u])) : win_add(a[u], q[u]);
          }
          win_store<V>(score + (long)c * S + idx, a);
        }
      }
    }
    win_store<V>(weight + idx, wacc);
    if constexpr (NCMAX > 0) {
#pragma unroll
      for (int c = 0; c < NCMAX; ++c)
        if (c < C) win_store<V>(score + (long)c * S + idx, acc[c]);
    }
  }
}

// label [s0][s1][s2] (int64) = arg-max over c of score[c] / weight (IEEE fp32 division) on the unpadded extent, which starts at `a` in
// the padded maps.  The lowest index wins among equals and a NaN beats every number (the first NaN wins), as torch.argmax has it.
// quot != nullptr: the quotients are written too, cropped, [C][s0][s1][s2]; quot may BE score when nothing is cropped (every thread then
// writes the elements it has read, hence no __restrict__ on the two).  label may be nullptr (quotients only).
// V = 4: s2, p2 and a2 multiples of 4, aligned pointers.
template <int V>
__global__ __launch_bounds__(256) void window_finalize_kernel(const float* score, const float* __restrict__ weight, long long* __restrict__ label,
                                                              float* quot, int C, WinExt p, WinExt a, WinExt s) {
  const int s2v = s.d2 / V;
  const long total = (long)s.d0 * s.d1 * s2v;
  const long S = (long)p.d0 * p.d1 * p.d2, U = (long)s.d0 * s.d1 * s.d2;
  for (long e = (long)blockIdx.x * blockDim.x + threadIdx.x; e < total; e += (long)gridDim.x * blockDim.x) {
    long t = e;
    const int z = (int)(t % s2v) * V;
    t /= s2v;
    const int y = (int)(t % s.d1), x = (int)(t / s.d1);
    const long pidx = ((long)(x + a.d0) * p.d1 + (y + a.d1)) * p.d2 + (z + a.d2), uidx = e * V;
    float wv[V], best[V];
    int bi[V];
    win_load<V>(weight + pidx, wv);
    for (int c = 0; c < C; ++c) {
      float q[V];
      win_load<V>(score + (long)c * S + pidx, q);
#pragma unroll
      for (int u = 0; u < V; ++u) {
        q[u] = q[u] / wv[u];
        if (c == 0 || (best[u] == best[u] && (q[u] != q[u] || q[u] > best[u]))) {
          best[u] = q[u];
          bi[u] = c;
        }
      }
      if (quot) win_store<V>(quot + (long)c * U + uidx, q);
    }
    if (label) {
#pragma unroll
      for (int u = 0; u < V; ++u) label[uidx + u] = (long long)bi[u];
    }
  }
}

}  // namespace icl
