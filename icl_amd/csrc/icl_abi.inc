// icl_abi.inc — the extern "C" launchers declared in include/icl_hip.h.
// Included by icl_hip.hip (gfx950 product build) after device_env_hip.h; tests/hipemu/icl_emu.cpp
// includes the same text after hipemu.h so that the launch geometry is exercised on the CPU too.

#include "kernels/common.h"
#include "kernels/norm.h"
#include "kernels/pool_resize.h"
#include "kernels/reduce.h"
#include "kernels/conv_mfma.h"
#include "kernels/conv_mfma_static.h"
#include "kernels/conv_mfma_flat.h"
#include "kernels/conv_bf16x3.h"
#include "kernels/conv_bf16x3_ws.h"
#include "kernels/conv_wgrad_tr.h"
#include "kernels/conv_wgrad_zs.h"
#include "kernels/conv_cin1.h"
#include "kernels/misc.h"
#include "kernels/loss.h"
#include "kernels/loss_point.h"
#include "kernels/optim.h"
#include "kernels/adamw.h"
#include "kernels/gradclip.h"
#include "kernels/winattn.h"
#include "kernels/linear_wgrad.h"
#include "kernels/token.h"
#include "kernels/gemm.h"
#include "kernels/datafeed.h"
#include "kernels/rankindex.h"
#include "kernels/prefix.h"
#include "kernels/intensity.h"
#include "kernels/qchain.h"
#include "kernels/metrics.h"
#include "kernels/metrics_surface.h"
#include "kernels/components.h"
#include "kernels/window.h"

#ifdef ICL_TWO_UNITS
// product build: this instantiation lives in icl_hip_noslp.hip (compiled with -fno-slp-vectorize; the reason is in that file's header)
namespace icl {
extern template __global__ void conv3d_bf16x3_fwd_ws_kernel<1, false, false>(const float*, const uint4*, const float*, float*, Bf3Geom);
}
#endif

#include <atomic>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace {

thread_local char g_err[512] = "";
thread_local char g_kernel[160] = "";  // name of the conv kernel instantiation chosen by the last launch (bench.py roofline)
// route of the last pooling / resize / depth-to-space launcher (kernels/pool_resize.h), for the tests: the kernel's name; the three-pass
// resize backward "x:<k>|y:<k>|z:<k>"; the depth-to-space pair the name + "+big_lds" / "+lds".  Not g_kernel: ops.py reads that one at the
// end of a timed convolution region.
thread_local char g_resample[192] = "";

void note_resample(const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_resample, sizeof(g_resample), fmt, ap);
  va_end(ap);
}

int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof(g_err), fmt, ap);
  va_end(ap);
  return code;
}

int check_launch(const char* what) {
  const int e = ICL_LAST_LAUNCH_ERROR();
  if (e != 0) return fail(-2, "%s: launch failed: %s", what, ICL_ERROR_STRING(e));
  return 0;
}

inline int round_up(int a, int b) { return (a + b - 1) / b * b; }
inline long cdivl(long a, long b) { return (a + b - 1) / b; }
inline bool aligned16(const void* p) { return ((uintptr_t)p & 15) == 0; }
inline int grid_for(long total, int block, int cap = 2048 * 4) {
  long g = cdivl(total, block);
  if (g < 1) g = 1;
  if (g > cap) g = cap;
  return (int)g;
}
// (Round 4, measured and dropped: leaving 8 / 16 / 32 of the 256 CUs free of persistent convolution workgroups, for the small dependent kernels
// of the aligner lanes that run beside the decoder's convolutions: 11.14 -> 11.17-11.20 / 11.27-11.30 / 11.57 ms per step.)
inline int largest_divisor_le(int n, int cap) {
  if (cap < 1) cap = 1;
  for (int d = cap < n ? cap : n; d >= 1; --d)
    if (n % d == 0) return d;
  return 1;
}

constexpr int kConvWaves = 4;
constexpr int kMaxDynLds = 64 * 1024;       // default dynamic-LDS ceiling
constexpr int kMaxDynLdsBig = 96 * 1024;    // with ICL_SET_MAX_DYN_LDS (wgrad tiles)
constexpr int kMaxDynLdsFwd = 76 * 1024;    // forward tiles: two workgroups per CU (register-limited anyway)

// Output-tile geometry: TX covers whole rows of narrow volumes, 16 voxels of wide ones; rows are staged as the
// 16-byte aligned span [x0-HX, x0+TX+HX) when W % 4 == 0 (vector staging).
void choose_tile(icl::ConvGeom& g, int ks, int target, bool vec) {
  const int pad = ks / 2;
  g.HX = pad ? (vec ? 4 : pad) : 0;
  g.TX = g.W >= 32 ? 16 : round_up(g.W, 4);
  g.PXL = g.TX + 2 * g.HX;
  g.TY = largest_divisor_le(g.H, 8);
  g.TZ = largest_divisor_le(g.D, target / (g.TX * g.TY));
}

void finish_tile(icl::ConvGeom& g, int ks, int ps_mod, int ps_of) {
  g.ntx = (g.W + g.TX - 1) / g.TX;
  g.nty = (g.H + g.TY - 1) / g.TY;
  g.ntz = (g.D + g.TZ - 1) / g.TZ;
  int ps = (g.TZ + ks - 1) * (g.TY + ks - 1) * g.PXL;
  while (ps % ps_of != ps_mod) ++ps;
  g.PS = ps;
}

// ---- 3x3x3 / 1x1x1 forward and input gradient: plan first, then launch ------------------------------------------------------------
// A plan is a value made from the shape and the environment switches alone — no tensor pointer, no stream.  The queries
// (icl_conv3d_fwd_ws_bytes, _presplit_ws_bytes, _stats_slots, _live_ok) read plans; the launch functions take a plan and the pointers
// and decide only what depends on the pointers.

struct ConvShape { int n, cin, cout, d, h, w; };
struct ConvArgs { const float* x; const float* wp; const float* bias; float* y; int64_t xbs, ybs; hipStream_t stream; };

// the planner's switches, read per call: the tests switch them
struct ConvEnv {
  int split;               // ICL_CONV_SPLIT (1); 0: exact-fp32 MFMA everywhere
  const char* min_vox;     // ICL_CONV_SPLIT_MIN: smallest volume of the split-product kernels (unset: 24^3; 12^3 / 6^3 on their flat tiles)
  int flat24, flat12, flat6;   // ICL_CONV_SPLIT_FLAT / _FLAT12 / _FLAT6 (1): the flat tiles of rows of 24 / 12 voxels and of the 6^3 volume (A/B)
  int ksplit;              // ICL_CONV_SPLIT_KSPLIT: 0: never split (A/B); n > 0: that many slices wherever the shape allows; unset (-1): cost model
  int cus;                 // ICL_CONV_SPLIT_KSPLIT_CUS (256): the CUs a launch is planned for (the deep backward shares the chip with the narrow
                           // update streams: optim.h sgd_factored_narrow_kernel)
  const char* force_tile;  // ICL_CONV_FORCE_TILE, tests only: "48" forces the 4x8x16 fp32 tile on small volumes, "28" the 2x8x16 one
};
inline int env_int(const char* name, int unset) { const char* e = getenv(name); return e ? atoi(e) : unset; }
ConvEnv conv_env() {
  const int cus = env_int("ICL_CONV_SPLIT_KSPLIT_CUS", 0);
  return {env_int("ICL_CONV_SPLIT", 1), getenv("ICL_CONV_SPLIT_MIN"), env_int("ICL_CONV_SPLIT_FLAT", 1), env_int("ICL_CONV_SPLIT_FLAT12", 1),
          env_int("ICL_CONV_SPLIT_FLAT6", 1), env_int("ICL_CONV_SPLIT_KSPLIT", -1), cus > 0 ? cus : 256, getenv("ICL_CONV_FORCE_TILE")};
}

inline icl::ConvGeom conv_geom(int cin, int cout, int d, int h, int w, int64_t xbs, int64_t ybs) {
  icl::ConvGeom g{};
  g.Cin = cin; g.Cout = cout;
  g.CinP = round_up(cin, 4); g.CoutP = round_up(cout, 16);
  g.D = d; g.H = h; g.W = w;
  g.x_bstride = xbs; g.y_bstride = ybs;
  return g;
}

// sum the split-K partial slabs (+bias) into y; no-op when the launch was not split
template <class Geom>
int splitk_reduce(const Geom& g, const float* bias, float* y, int n, int64_t ybs, hipStream_t stream) {
  if (g.ksplit <= 1) return 0;
  const long dhw = (long)g.D * g.H * g.W, per = (long)g.Cout * dhw;
  ICL_LAUNCH(icl::splitk_reduce_kernel, dim3(grid_for((long)n * per, 256)), dim3(256), 0, stream, (const float*)g.slab, bias, y, g.ksplit, n, per,
             dhw, (long)ybs);
  return check_launch("splitk_reduce");
}

// XCD-aware workgroup order (kernels/conv_mfma.h xcd_chunked): needs gridDim.x % 8 == 0.
inline int xcd_remap_for(long grid_x) { return (grid_x % 8 == 0 && grid_x >= 64) ? 1 : 0; }

// Cin-chunk split for launches with too few workgroups to fill 256 CUs
inline int choose_ksplit(long base, int nchunks) {
  int ksplit = 1;
  // ~two workgroups per CU: measured on the 24^3 / 12^3 layers (tools/conv_one.py, batch 2): 64..192->64 @24^3 run at 73-96
  // TFLOP/s with three splits (432 workgroups) against 63-67 unsplit (144); 128..384->128 @12^3 at 61-79 with eight against
  // 55-66 with four
  if (base <= 320) ksplit = (int)((480 + base / 2) / base);
  if (ksplit > nchunks) ksplit = nchunks;
  if (ksplit < 1) ksplit = 1;
  return ksplit;
}

// ---- the fp32 MFMA kernels: flat full-row tiles, compile-time tiles, the generic kernel ------------------------------------------
struct Fp32Plan {
  int rc;                        // -1: no tiling covers the shape (g_err has the text)
  ConvShape s;
  icl::ConvGeom g;               // the tile and its LDS layout; strides, slab, the split taken and the workgroup order come with the pointers
  int nbt, ntiles, ctiles;       // cout blocks per workgroup; grid = (ntiles * ksplit, ctiles, n)
  size_t lds;
  int ksplit;                    // the split over the Cin chunks this grid wants: taken when the call brings a workspace
  int64_t slab_bytes;            // ... of this size
  int (*go)(const Fp32Plan&, const ConvArgs&, float* slab);     // the instantiation that runs the plan
};

// what the tile choice leaves to do: the grid, the wanted k-split, the LDS bytes
void fp32_plan_grid(Fp32Plan& p, int taps) {
  const icl::ConvGeom& g = p.g;
  const int nb = p.nbt * 16;
  p.ntiles = g.ntx * g.nty * g.ntz;
  p.ctiles = (g.CoutP + nb - 1) / nb;
  p.ksplit = choose_ksplit((long)p.ntiles * p.ctiles * p.s.n, g.CinP / g.KC);
  p.slab_bytes = p.ksplit > 1 ? (int64_t)p.ksplit * p.s.n * g.Cout * g.D * g.H * g.W * 4 : 0;
  p.lds = (size_t)g.KC * (g.PS + taps * nb) * 4;
}

// the plan's geometry with the pointers of a call; no workspace supplied: run unsplit
inline icl::ConvGeom fp32_launch_geom(const Fp32Plan& p, const ConvArgs& a, float* slab) {
  icl::ConvGeom g = p.g;
  g.x_bstride = a.xbs; g.y_bstride = a.ybs; g.slab = slab;
  g.ksplit = slab ? p.ksplit : 1;
  return g;
}

// compile-time tiles: FwdTile (conv_mfma_static.h, XCD-aware workgroup order) and the full-row FlatTile (conv_mfma_flat.h)
template <int NBT, class TC, bool FLAT>
int conv_fwd_tile_go(const Fp32Plan& p, const ConvArgs& a, float* slab) {
  icl::ConvGeom g = fp32_launch_geom(p, a, slab);
  const dim3 grid(p.ntiles * g.ksplit, p.ctiles, p.s.n);
  if constexpr (FLAT) {
    if (p.lds > (size_t)kMaxDynLds) ICL_SET_MAX_DYN_LDS((icl::conv3d_mfma_fwd_flat_kernel<NBT, TC>), kMaxDynLdsBig);
    ICL_LAUNCH((icl::conv3d_mfma_fwd_flat_kernel<NBT, TC>), grid, dim3(256), p.lds, a.stream, a.x, a.wp, a.bias, a.y, g);
    snprintf(g_kernel, sizeof(g_kernel), "conv3d_mfma_fwd_flat_kernel<%d, icl::FlatTile<%d, %d, %d, %d, %s> >", NBT, TC::TZ, TC::TY, TC::TX, TC::KC, TC::VEC ? "true" : "false");
  } else {
    if (p.lds > (size_t)kMaxDynLds) ICL_SET_MAX_DYN_LDS((icl::conv3d_mfma_fwd_static_kernel<NBT, TC>), kMaxDynLdsBig);
    g.remap = xcd_remap_for((long)p.ntiles * g.ksplit);
    ICL_LAUNCH((icl::conv3d_mfma_fwd_static_kernel<NBT, TC>), grid, dim3(256), p.lds, a.stream, a.x, a.wp, a.bias, a.y, g);
    snprintf(g_kernel, sizeof(g_kernel), "conv3d_mfma_fwd_static_kernel<%d, icl::FwdTile<%d, %d, %d> >", NBT, TC::TZ, TC::TY, TC::KC);
  }
  const int rc = check_launch(FLAT ? "conv3d_fwd_flat" : "conv3d_fwd_static");
  return rc ? rc : splitk_reduce(g, a.bias, a.y, p.s.n, a.ybs, a.stream);
}

template <int NBT, class TC, bool FLAT>
Fp32Plan plan_tile(const ConvShape& s) {
  Fp32Plan p{};
  p.s = s; p.nbt = NBT;
  icl::ConvGeom& g = p.g = conv_geom(s.cin, s.cout, s.d, s.h, s.w, 0, 0);
  g.TZ = TC::TZ; g.TY = TC::TY; g.TX = TC::TX; g.KC = TC::KC; g.PS = TC::PS; g.PXL = TC::PXL; g.HX = TC::HX; g.CPP = TC::CPP;
  g.ntx = (g.W + TC::TX - 1) / TC::TX;
  g.nty = (g.H + TC::TY - 1) / TC::TY;
  g.ntz = (g.D + TC::TZ - 1) / TC::TZ;
  fp32_plan_grid(p, TC::T);
  p.go = conv_fwd_tile_go<NBT, TC, FLAT>;
  return p;
}

// narrow volumes (the deep U-Net levels): full-row tiles; false when not applicable
bool plan_flat(const ConvShape& s, Fp32Plan& p) {
  if ((round_up(s.cin, 4) % 8) != 0 || s.cout <= 16) return false;
  const bool nb48 = (round_up(s.cout, 16) % 48) == 0;
  if (s.w == 24 && (s.h % 8) == 0) p = nb48 ? plan_tile<3, icl::FlatTile<2, 8, 24, 4, true>, true>(s) : plan_tile<2, icl::FlatTile<2, 8, 24, 8, true>, true>(s);
  else if (s.w == 12 && (s.h % 4) == 0) p = nb48 ? plan_tile<3, icl::FlatTile<4, 4, 12, 4, true>, true>(s) : plan_tile<2, icl::FlatTile<4, 4, 12, 8, true>, true>(s);
  else if (s.w == 6 && s.h == 6 && !nb48) p = plan_tile<2, icl::FlatTile<6, 6, 6, 8, false>, true>(s);
  else return false;
  return true;
}

template <int TZ, int TY>
Fp32Plan plan_static_tile(const ConvShape& s, int nbt) {
  // KC = 4 channels per chunk: 6-14 % faster than 8 on every 96^3 / 48^3 shape (half the staging registers and LDS -> more waves per
  // SIMD; DESIGN.md section 4).  The 8-channel instantiations are gone (round 5: six kernels nothing launched).
  if (nbt == 1) return plan_tile<1, icl::FwdTile<TZ, TY, 4>, false>(s);
  if (nbt == 2) return plan_tile<2, icl::FwdTile<TZ, TY, 4>, false>(s);
  return plan_tile<3, icl::FwdTile<TZ, TY, 4>, false>(s);
}

// false when the shape is not covered by a static tile (the generic kernel takes it)
bool plan_static(const ConvShape& s, const ConvEnv& e, Fp32Plan& p) {
  if ((s.w % 4) != 0 || s.w < 12 || (s.h % 4) != 0) return false;
  const int coutP = round_up(s.cout, 16);
  const int nbt = s.cout <= 16 ? 1 : (coutP % 48 == 0 ? 3 : 2);
  if ((s.h % 8) == 0) {
    const int ctiles = (coutP + nbt * 16 - 1) / (nbt * 16);
    const long big = (long)((s.d + 3) / 4) * (s.h / 8) * ((s.w + 15) / 16) * ctiles * s.n;
    const char* force = e.force_tile;
    // 32/48-cout blocks: the 2x8x16 tile (4 accumulator row groups per wave, <= 36 KB LDS -> 4 workgroups per CU) measures
    // 122-136 TFLOP/s on the 96^3 layers against 118-129 for 4x8x16; 16-cout blocks are 2 % faster on 4x8x16 (tools/conv_one.py)
    if (nbt >= 2 && !(force && force[0] == '4')) p = plan_static_tile<2, 8>(s, nbt);
    else if (force && force[0] == '2' && force[1] == '8') p = plan_static_tile<2, 8>(s, nbt);
    else if (big >= 512 || (force && force[0] == '4' && force[1] == '8')) p = plan_static_tile<4, 8>(s, nbt);
    else p = plan_static_tile<2, 8>(s, nbt);
  } else {
    p = plan_static_tile<4, 4>(s, nbt);
  }
  return true;
}

template <int KS, int NBT, bool VEC>
int conv_fwd_generic_go(const Fp32Plan& p, const ConvArgs& a, float* slab) {
  const icl::ConvGeom g = fp32_launch_geom(p, a, slab);
  if (p.lds > (size_t)kMaxDynLds) ICL_SET_MAX_DYN_LDS((icl::conv3d_mfma_fwd_kernel<KS, NBT, 8, kConvWaves, VEC>), kMaxDynLdsBig);
  ICL_LAUNCH((icl::conv3d_mfma_fwd_kernel<KS, NBT, 8, kConvWaves, VEC>), dim3(p.ntiles * g.ksplit, p.ctiles, p.s.n), dim3(kConvWaves * 64), p.lds,
             a.stream, a.x, a.wp, a.bias, a.y, g);
  snprintf(g_kernel, sizeof(g_kernel), "conv3d_mfma_fwd_kernel<%d, %d, 8, 4, %s>", KS, NBT, VEC ? "true" : "false");
  const int rc = check_launch("conv3d_fwd");
  return rc ? rc : splitk_reduce(g, a.bias, a.y, p.s.n, a.ybs, a.stream);
}

// any extent, any channel count: run-time tiles (kernels/conv_mfma.h)
template <int KS>
Fp32Plan plan_generic(const ConvShape& s) {
  Fp32Plan p{};
  p.s = s;
  icl::ConvGeom& g = p.g = conv_geom(s.cin, s.cout, s.d, s.h, s.w, 0, 0);
  const bool vec = KS == 1 && (s.w % 4) == 0;      // 16-byte loads: instantiated for 1x1x1 only (see below)
  choose_tile(g, KS, 512, vec);
  finish_tile(g, KS, 16, 32);
  constexpr int T = KS * KS * KS;
  p.nbt = s.cout <= 16 ? 1 : (g.CoutP % 48 == 0 ? 3 : 2);
  const int nb = p.nbt * 16;
  const int per_ch = (g.TZ + KS - 1) * (g.TY + KS - 1) * (g.PXL / (vec ? 4 : 1));
  for (int cand = 16; cand >= 4 && !g.KC; cand >>= 1) {
    if (g.CinP % cand) continue;
    if ((size_t)cand * (g.PS + T * nb) * 4 > (size_t)kMaxDynLdsFwd) continue;
    if (T * cand * (nb / 4) > icl::kWX * kConvWaves * 64) continue;
    const int cpp = cand / 4 > 1 ? cand / 4 : 1;
    if (cpp * per_ch > icl::kJX * kConvWaves * 64) continue;
    g.KC = cand;
    g.CPP = cpp;
  }
  const int mt = g.TZ * g.TY * g.TX;
  if (!g.KC) p.rc = fail(-1, "conv3d_fwd: no LDS tiling for %dx%dx%d cin %d cout %d", s.d, s.h, s.w, s.cin, s.cout);
  else if (mt > kConvWaves * 8 * 16) p.rc = fail(-1, "conv3d_fwd: tile of %d voxels too large", mt);
  if (p.rc) return p;
  fp32_plan_grid(p, T);
  // (the 16-byte-load instantiations of this generic kernel exist for 1x1x1 only: every 3x3x3 shape of the models runs on the split-product,
  // flat or compile-time-tile kernels above, and what falls through to here — odd extents, channel counts that are no multiple of 4 — is
  // not worth 135 KB of code object)
#define ICL_FWD_CASE(NBT_) (vec ? conv_fwd_generic_go<KS, NBT_, KS == 1> : conv_fwd_generic_go<KS, NBT_, false>)
  if (p.nbt == 1) p.go = ICL_FWD_CASE(1);
  else if (p.nbt == 2) p.go = ICL_FWD_CASE(2);
  else p.go = ICL_FWD_CASE(3);
#undef ICL_FWD_CASE
  return p;
}

// the fp32 plan of a shape: what runs where the split-product kernels do not
template <int KS>
Fp32Plan plan_conv_fp32(const ConvShape& s, const ConvEnv& e) {
  Fp32Plan p{};
  if (KS == 3 && (plan_flat(s, p) || plan_static(s, e, p))) return p;
  return plan_generic<KS>(s);
}

// workgroups = pairs * n * split ~ two per CU; each (split, batch) pair owns one partial-sum slab
inline int wgrad_max_split(int pairs, int n) {
  int s = 512 / (pairs * n);      // 512 workgroups = two per CU
  return s < 1 ? 1 : s;
}

constexpr int kWgradWaveGroups = 2;   // 8-wave workgroups: two wave groups, each with its own slab

// Live batch (icl_conv3d_wgrad_live): samples [n_live, n) of dY are exactly zero (n_live == n: no live batch).  The tile-list kernels keep the plan of the batch of n
// — tiles are numbered sample-outermost, so the workgroups that own live tiles are a prefix of the grid — launch that prefix only and
// write the slabs of the rest as zeros (what those workgroups would have written): the reduction sums the same slabs in the same order,
// the weight gradient is bit for bit the full call's.  Every other weight-gradient kernel runs the whole batch.
thread_local int g_wgrad_grid[2] = {0, 0};      // workgroups launched / planned by the last tile-list weight-gradient launch (tests)
thread_local char g_kernel_live_fwd[160] = "";  // kernel of the last live input-gradient launch (icl_conv3d_fwd*_live), for the tests

// workgroups of a tile-list launch that own a live tile; zeros to the slabs of the others
inline int wgrad_live_prefix(float* gwp, int nsplit, int ntiles, int tiles_per_wg, int n, int n_live, long slab_elems, hipStream_t stream) {
  g_wgrad_grid[0] = g_wgrad_grid[1] = nsplit;
  if (n_live >= n) return nsplit;
  const long live_tiles = (long)n_live * (ntiles / n);
  int gx = (int)cdivl(live_tiles, tiles_per_wg);
  if (gx >= nsplit) return nsplit;
  if (gx < 1) gx = 1;
  ICL_MEMSET_ASYNC(gwp + (size_t)gx * slab_elems, 0, (size_t)(nsplit - gx) * slab_elems * sizeof(float), stream);
  g_wgrad_grid[0] = gx;
  return gx;
}

template <class TC, int WV, int NCB, int TGN = 4>
int conv_wgrad_static_go(const float* x, const float* gy, float* gwp, icl::ConvGeom g, int n, int* nslabs, hipStream_t stream) {
  g.TZ = TC::TZ; g.TY = TC::TY; g.TX = TC::TX; g.KC = 16; g.PS = TC::PS; g.PXL = TC::PXL; g.HX = TC::HX; g.CPP = TC::CPP; g.ksplit = 1;
  g.ntx = (g.W + TC::TX - 1) / TC::TX;
  g.nty = (g.H + TC::TY - 1) / TC::TY;
  g.ntz = (g.D + TC::TZ - 1) / TC::TZ;
  const int pairs = ((g.CoutP + 16 * NCB - 1) / (16 * NCB)) * ((g.CinP + 15) / 16);
  const int ntiles = g.ntx * g.nty * g.ntz;
  int nsplit = wgrad_max_split(pairs, n);
  if (nsplit > ntiles) nsplit = ntiles;
  if (nsplit >= 64) nsplit = nsplit / 8 * 8;   // multiple of 8 (rounded down: the workspace is sized for the maximum): XCD-aware order
  g.remap = xcd_remap_for(nsplit);
  *nslabs = nsplit * n * (WV / TGN);
  const size_t lds = (size_t)(16 * TC::PS + 16 * NCB * TC::MTP) * 4;
  ICL_SET_MAX_DYN_LDS((icl::conv3d_mfma_wgrad_static_kernel<TC, WV, NCB, TGN>), kMaxDynLdsBig);
  ICL_LAUNCH((icl::conv3d_mfma_wgrad_static_kernel<TC, WV, NCB, TGN>), dim3(nsplit, pairs, n), dim3(64 * WV), lds, stream, x, gy, gwp, g);
  if (TGN == 4) snprintf(g_kernel, sizeof(g_kernel), "conv3d_mfma_wgrad_static_kernel<icl::WgradTileT<%d, %d>, %d, %d>", TC::TZ, TC::TY, WV, NCB);
  else snprintf(g_kernel, sizeof(g_kernel), "conv3d_mfma_wgrad_static_kernel<icl::WgradTileT<%d, %d>, %d, %d, %d>", TC::TZ, TC::TY, WV, NCB, TGN);
  return check_launch("conv3d_wgrad_static");
}

// Split-product weight gradient (kernels/conv_wgrad_tr.h): 2 x 4 x 16 tiles in two LDS buffers, transposing LDS
// reads, eight waves (k-step x tap half).  NCB = 2 when the padded Cout is a multiple of 32, else one cout block per workgroup column.
template <int NCB>
int conv_wgrad_tr_go(const float* x, const float* gy, float* gwp, const icl::ConvGeom& g, int n, int n_live, int* nslabs, hipStream_t stream) {
  typedef icl::WgTrT<NCB> C;
  icl::Bf3WGeom w{};
  w.Cin = g.Cin; w.Cout = g.Cout; w.CinP = g.CinP; w.CoutP = g.CoutP; w.D = g.D; w.H = g.H; w.W = g.W;
  w.ntz = (g.D + C::TZ - 1) / C::TZ; w.nty = (g.H + C::TY - 1) / C::TY; w.ntx = (g.W + C::TX - 1) / C::TX;
  w.ntiles = n * w.ntz * w.nty * w.ntx;
  const int pairs = ((g.CoutP + 16 * NCB - 1) / (16 * NCB)) * ((g.CinP + 15) / 16);
  const int pairs_ws = ((g.CoutP + 47) / 48) * ((g.CinP + 15) / 16);
  const int cap = n * wgrad_max_split(pairs_ws, n) * kWgradWaveGroups;
  int nsplit = 256 / pairs > 0 ? 256 / pairs : 1;        // one 512-thread workgroup per CU, all resident
  if (nsplit > cap) nsplit = cap;
  if (nsplit > w.ntiles) nsplit = w.ntiles;
  w.tiles_per_wg = (w.ntiles + nsplit - 1) / nsplit;
  nsplit = (w.ntiles + w.tiles_per_wg - 1) / w.tiles_per_wg;
  w.x_bstride = g.x_bstride; w.gy_bstride = g.y_bstride;
  *nslabs = nsplit;
  { const char* e = getenv("ICL_WGRAD_TR_DBG"); w.dbg = e ? atoi(e) : 0; }
  ICL_SET_MAX_DYN_LDS((icl::conv3d_wgrad_tr_kernel<NCB>), 160 * 1024);
  const int gx = wgrad_live_prefix(gwp, nsplit, w.ntiles, w.tiles_per_wg, n, n_live, 27L * w.CinP * w.CoutP, stream);
  ICL_LAUNCH((icl::conv3d_wgrad_tr_kernel<NCB>), dim3(gx, pairs), dim3(512), C::LDS_BYTES, stream, x, gy, gwp, w);
  snprintf(g_kernel, sizeof(g_kernel), "conv3d_wgrad_tr_kernel<%d>", NCB);
  return check_launch("conv3d_wgrad_tr");
}

// Split-product weight gradient walking z-columns of 1 x 8 x 16 tiles with a ring of halo planes in LDS (kernels/conv_wgrad_zs.h):
// a phase stages 180 + 128 NCB positions instead of 432 + 128 NCB.  Same workspace bound and slab format as conv_wgrad_tr_go.
template <int NCB>
int conv_wgrad_zs_go(const float* x, const float* gy, float* gwp, const icl::ConvGeom& g, int n, int n_live, int* nslabs, hipStream_t stream) {
  // one cout block: ten waves — the 360 + 256 staging items of a phase are exactly one round of 640 threads (waves 8 and 9 only stage)
  constexpr int NW = NCB == 1 ? 10 : 8;
  typedef icl::WgZsT<NCB, NW> C;
  icl::Bf3WGeom w{};
  w.Cin = g.Cin; w.Cout = g.Cout; w.CinP = g.CinP; w.CoutP = g.CoutP; w.D = g.D; w.H = g.H; w.W = g.W;
  w.ntz = g.D; w.nty = (g.H + C::TY - 1) / C::TY; w.ntx = (g.W + C::TX - 1) / C::TX;
  w.ntiles = n * w.ntz * w.nty * w.ntx;
  const int pairs = ((g.CoutP + 16 * NCB - 1) / (16 * NCB)) * ((g.CinP + 15) / 16);
  const int pairs_ws = ((g.CoutP + 47) / 48) * ((g.CinP + 15) / 16);
  const int cap = n * wgrad_max_split(pairs_ws, n) * kWgradWaveGroups;
  int nsplit = 256 / pairs > 0 ? 256 / pairs : 1;        // one 512-thread workgroup per CU, all resident
  if (nsplit > cap) nsplit = cap;
  if (nsplit > w.ntiles) nsplit = w.ntiles;
  { const char* e = getenv("ICL_WGRAD_ZS_MAX_WGS"); if (e && atoi(e) > 0 && atoi(e) < nsplit) nsplit = atoi(e); }   // tests only: long runs on small volumes
  w.tiles_per_wg = (w.ntiles + nsplit - 1) / nsplit;
  nsplit = (w.ntiles + w.tiles_per_wg - 1) / w.tiles_per_wg;
  w.x_bstride = g.x_bstride; w.gy_bstride = g.y_bstride;
  *nslabs = nsplit;
  { const char* e = getenv("ICL_WGRAD_TR_DBG"); w.dbg = e ? atoi(e) : 0; }
  ICL_SET_MAX_DYN_LDS((icl::conv3d_wgrad_zs_kernel<NCB, NW>), 160 * 1024);
  const int gx = wgrad_live_prefix(gwp, nsplit, w.ntiles, w.tiles_per_wg, n, n_live, 27L * w.CinP * w.CoutP, stream);
  ICL_LAUNCH((icl::conv3d_wgrad_zs_kernel<NCB, NW>), dim3(gx, pairs), dim3(C::NT), C::LDS_BYTES, stream, x, gy, gwp, w);
  snprintf(g_kernel, sizeof(g_kernel), "conv3d_wgrad_zs_kernel<%d, %d>", NCB, NW);
  return check_launch("conv3d_wgrad_zs");
}

// Weight gradient on split products (kernels/conv_wgrad_tr.h, conv_wgrad_zs.h).  Returns 1 when the shape is left to the fp32 kernels.
// ICL_CONV_SPLIT=0 / ICL_WGRAD_SPLIT=0: exact-fp32 MFMA weight gradients.
int conv_wgrad_split(const float* x, const float* gy, float* gwp, const icl::ConvGeom& g, int n, int n_live, int* nslabs, hipStream_t stream) {
  const char* e_on = getenv("ICL_CONV_SPLIT");
  const char* e_min = getenv("ICL_CONV_SPLIT_MIN");
  const char* e_w = getenv("ICL_WGRAD_SPLIT");
  const int on = (e_on ? atoi(e_on) : 1) && (e_w ? atoi(e_w) : 1) > 0;
  // from 12^3 on (round 3; batch 2, fp32 kernel in brackets): 128->128 @12^3 41.7 us (66.8), 256->128 61.1 (99.8), 64->128 29.8 (46.8);
  // 64->64 @24^3 50 (102); 16->16 @96^3 153 (274), 48->16 469 (770), 32->32 @48^3 76 (143)
  const long min_vox = e_min ? atol(e_min) : 12L * 12 * 12;
  if (!on || (long)g.D * g.H * g.W < min_vox || (long)g.D * g.H * g.W * 192 > (1L << 31) || !aligned16(gwp)) return 1;
  const bool two = g.CoutP % 32 == 0;
  // z-column walk (round 5; batch 2, against the 2 x 4 x 16-tile kernel: 16->16 @96^3 148 vs 170 us, 48->16 436 vs 520, 32->16 282 vs 341,
  // 48->48 1038 vs 1314; 96->32 @48^3 183 vs 194, 32->32 77 vs 76, 64->64 @24^3 50 vs 51): rows of 8 must tile H — the 12^3 / 6^3 levels
  // keep the 2 x 4 x 16 tiles.  Three cout blocks per workgroup for the 48-multiples that are not 32-multiples (SwinUNETR's decoder at
  // 96^3: x is staged once per 48 couts instead of once per 16).  ICL_WGRAD_ZS=0: the 2 x 4 x 16-tile kernel everywhere (A/B).
  const char* e_zs = getenv("ICL_WGRAD_ZS");
  if ((e_zs ? atoi(e_zs) : 1) && g.H % 8 == 0 && g.D >= 8) {
    if (!two && g.CoutP % 48 == 0) return conv_wgrad_zs_go<3>(x, gy, gwp, g, n, n_live, nslabs, stream);
    return two ? conv_wgrad_zs_go<2>(x, gy, gwp, g, n, n_live, nslabs, stream) : conv_wgrad_zs_go<1>(x, gy, gwp, g, n, n_live, nslabs, stream);
  }
  return two ? conv_wgrad_tr_go<2>(x, gy, gwp, g, n, n_live, nslabs, stream) : conv_wgrad_tr_go<1>(x, gy, gwp, g, n, n_live, nslabs, stream);
}

int conv_wgrad_static(const float* x, const float* gy, float* gwp, const icl::ConvGeom& g, int n, int n_live, int* nslabs, hipStream_t stream) {
  {   // the split-product kernels check their own shape conditions (the round-3 kernel takes any extent)
    const int rc = conv_wgrad_split(x, gy, gwp, g, n, n_live, nslabs, stream);
    if (rc != 1) return rc;
  }
  if ((g.W % 4) != 0 || g.W < 12 || (g.H % 4) != 0) return 1;
  // 48- / 32-cout blocks on a 2x4x16 tile: each staged x value feeds three / two MFMAs
  if (g.CoutP % 48 == 0) return conv_wgrad_static_go<icl::WgradTileT<2, 4>, 4, 3>(x, gy, gwp, g, n, nslabs, stream);
  if (g.CoutP % 32 == 0) return conv_wgrad_static_go<icl::WgradTileT<2, 4>, 4, 2>(x, gy, gwp, g, n, nslabs, stream);
  // one cout block: 8 waves x 8 tap groups (124 registers, no spills, four waves per SIMD): 79 vs 74 TFLOP/s on 16->16 @96^3,
  // 92 vs 86 on 48->16; with two / three cout blocks the same split spills (10 / 69 registers) and is equal / slower
  return conv_wgrad_static_go<icl::WgradTileT<4, 4>, 8, 1, 8>(x, gy, gwp, g, n, nslabs, stream);
}

// Split over the channel chunks for the split-product launches of the deep levels (round 6).  `base` workgroups of `nchunks` chunk
// items each on `slots` resident workgroups, `chunk_us` per item: the split with the smallest estimated time — makespan in chunk items
// plus, for k > 1 slices, the reduction launch and k slabs of the output written and read back (~3 TB/s at these sizes).
inline int choose_ksplit_bf3(long base, int nchunks, int slots, double chunk_us, double out_bytes) {
  int best = 1;
  double best_t = (double)(cdivl(base, slots) * nchunks) * chunk_us;
  for (int k = 2; k <= nchunks && k <= 16; ++k) {
    const double t = (double)(cdivl(base * k, slots) * cdivl(nchunks, k)) * chunk_us + 8.0 + k * out_bytes * 2.0 / 3.0e6;
    if (t < best_t) { best = k; best_t = t; }
  }
  return best;
}

template <int NBT>
int conv_fwd_split_go(const float* x, const float* wp, const float* bias, float* y, uint4* wsplit, const icl::Bf3Geom& g,
                      hipStream_t stream, int flat = 0) {
  if (wp) {      // wp == nullptr: wsplit already holds the split weights (icl_conv3d_fwd_presplit)
    const long items = (long)g.nchunks * 3 * 2 * icl::Bf3::SLOTS * g.CoutP;
    ICL_LAUNCH(icl::conv_bf16x3_split_weights_kernel, dim3(grid_for(items, 256, 512)), dim3(256), 0, stream, wp, wsplit, g.CinP, g.CoutP,
               g.nchunks);
    int rc = check_launch("conv3d_split_weights");
    if (rc) return rc;
  }
  const size_t lds = flat == 12 ? icl::Bf3F12::lds_bytes(NBT, NBT == 1 ? 3 : 1)
                     : flat == 6 ? icl::Bf3F6::lds_bytes(NBT, NBT == 1 ? 3 : 1)
                     : flat   ? icl::Bf3F24::lds_bytes(NBT, NBT == 1 ? 3 : 1) : icl::Bf3T<8>::lds_bytes(NBT, NBT == 1 ? 3 : 1);
  // g.wgs: a multiple of 8 (one tile list per XCD), from split_geom; split launches: one tile per workgroup, grid.z slices
  const dim3 grid(g.wgs, (g.CoutP + 16 * NBT - 1) / (16 * NBT), g.ksplit > 1 ? g.ksplit : 1);
  // One cout block on 4 x 8 x 16 tiles (round 4): eight consumer waves + four loader waves (kernels/conv_bf16x3_ws.h), 1.10-1.18x the
  // single-role kernel on the 16-cout layers at 96^3 (16->16 130 vs 147-154 us, 48->16 370 vs 408, 32->16 256 vs 286; bit-identical
  // outputs).  Everything else — two / three cout blocks, rows of 24 voxels (flat tiles) — runs the single-role kernel.
  if (NBT == 1 && !flat) {
    ICL_SET_MAX_DYN_LDS((icl::conv3d_bf16x3_fwd_ws_kernel<1, false>), 160 * 1024);
    ICL_LAUNCH((icl::conv3d_bf16x3_fwd_ws_kernel<1, false>), grid, dim3(768), icl::Bf3T<8>::lds_bytes(1, 3), stream, x, (const uint4*)wsplit, bias, y, g);
    snprintf(g_kernel, sizeof(g_kernel), "conv3d_bf16x3_fwd_ws_kernel<1>");
    return check_launch("conv3d_fwd_split_ws");
  }
  if (flat == 12 || flat == 6) {
    if constexpr (NBT == 2) {
      if (flat == 12) {
        ICL_SET_MAX_DYN_LDS((icl::conv3d_bf16x3_fwd_kernel<2, 4, 60, true>), 160 * 1024);
        ICL_LAUNCH((icl::conv3d_bf16x3_fwd_kernel<2, 4, 60, true>), grid, dim3(256), lds, stream, x, (const uint4*)wsplit, bias, y, g);
        snprintf(g_kernel, sizeof(g_kernel), "conv3d_bf16x3_fwd_kernel<2, 4, 60, flat12>");
      } else {
        ICL_SET_MAX_DYN_LDS((icl::conv3d_bf16x3_fwd_kernel<2, 6, 60, true>), 160 * 1024);
        ICL_LAUNCH((icl::conv3d_bf16x3_fwd_kernel<2, 6, 60, true>), grid, dim3(512), lds, stream, x, (const uint4*)wsplit, bias, y, g);
        snprintf(g_kernel, sizeof(g_kernel), "conv3d_bf16x3_fwd_kernel<2, 6, 60, flat6>");
      }
    } else {
      return fail(-1, "conv3d_fwd_split: rows of 12 / 6 voxels run with two cout blocks per workgroup");
    }
  } else if (flat) {
    ICL_SET_MAX_DYN_LDS((icl::conv3d_bf16x3_fwd_kernel<NBT, 8, 60, true>), 160 * 1024);
    ICL_LAUNCH((icl::conv3d_bf16x3_fwd_kernel<NBT, 8, 60, true>), grid, dim3(512), lds, stream, x, (const uint4*)wsplit, bias, y, g);
    snprintf(g_kernel, sizeof(g_kernel), "conv3d_bf16x3_fwd_kernel<%d, 8, 60, flat24>", NBT);
  } else if constexpr (NBT > 1) {
    ICL_SET_MAX_DYN_LDS((icl::conv3d_bf16x3_fwd_kernel<NBT, 8, 60>), 160 * 1024);
    ICL_LAUNCH((icl::conv3d_bf16x3_fwd_kernel<NBT, 8, 60>), grid, dim3(512), lds, stream, x, (const uint4*)wsplit, bias, y, g);
    snprintf(g_kernel, sizeof(g_kernel), "conv3d_bf16x3_fwd_kernel<%d, 8, 60>", NBT);
  }
  const int rc = check_launch("conv3d_fwd_split");
  return rc ? rc : splitk_reduce(g, bias, y, g.nbatch, g.y_bstride, stream);
}

// ---- the split-product plan and its launch ---------------------------------------------------------------------------------------
struct SplitPlan {
  bool ok;                       // the shape runs on the split-product kernels; a call is handed back only for what its pointers say
  ConvShape s;
  int flat;                      // tiles: 0: 4 x 8 x 16; 24 / 12: flat rows of that many voxels; 6: the whole 6^3 volume
  int nbt;                       // cout blocks per workgroup
  int ksplit;                    // slices over the channel chunks the cost model wants (1: none); taken when the call brings a slab
  int64_t w_bytes, slab_bytes;   // the split weights, (Cin / 16) x 3 dz planes x 60 CoutP slots of 16 bytes; the slabs of the slices
  int slots;                     // statistics slots per (sample, channel); 0 where the epilogue cannot give them
  icl::Bf3Geom g;                // of the launch with `ksplit` slices; strides, slab and statistics come with the pointers
};

// The geometry of a split-product launch with `ksplit` slices, all but the pointers and strides.
icl::Bf3Geom split_geom(const ConvShape& s, int flat, int ksplit) {
  icl::Bf3Geom g{};
  g.Cin = s.cin; g.Cout = s.cout; g.CinP = round_up(s.cin, 4); g.CoutP = round_up(s.cout, 16);
  g.D = s.d; g.H = s.h; g.W = s.w;
  if (flat == 6) { g.ntz = g.nty = g.ntx = 1; }
  else if (flat == 12) { g.ntz = s.d / icl::Bf3F12::TZ; g.nty = s.h / icl::Bf3F12::TY; g.ntx = 1; }
  else if (flat) { g.ntz = (s.d + icl::Bf3F24::TZ - 1) / icl::Bf3F24::TZ; g.nty = (s.h + icl::Bf3F24::TY - 1) / icl::Bf3F24::TY; g.ntx = 1; }
  else { g.ntz = (s.d + 3) / 4; g.nty = (s.h + 7) / 8; g.ntx = (s.w + 15) / 16; }
  g.ntiles = s.n * g.ntz * g.nty * g.ntx;
  g.nchunks = s.cin / 16;
  g.nbatch = s.n;
  g.flags = g.CoutP % 48 == 0 ? 2 : 0;      // non-temporal output stores for three cout blocks (kernels/conv_bf16x3.h)
  // the workgroup count along x, computed here and nowhere else: the launch grid AND the statistics slots per (sample, channel) that the
  // caller sized its buffer for (ADVICE round 4: the two must not be separate formulas)
  g.wgs = g.ntiles < 256 ? (g.ntiles + 7) / 8 * 8 : 256;
  if (ksplit > 1) {      // one tile per workgroup, grid.z slices, raw partial sums into the slab; no statistics from the epilogue
    g.ksplit = ksplit; g.slab_stride = (long)s.n * s.cout * s.d * s.h * s.w;
    g.flags = 4;           // (plain stores: the slab is read back at once)
    g.wgs = g.ntiles;
  }
  return g;
}

// InstanceNorm statistics from the epilogue (kernels/conv_bf16x3.h bf3_stats_*): one summary per (sample, channel, workgroup), g.wgs slots
// (the normalisation's `nchunks`).  0: a split launch, or a workgroup's tile list would span two samples — a workgroup walks tiles of
// ONE XCD's contiguous eighth of the tile list: its summary belongs to one sample iff no eighth spans two.
inline int split_stats_slots(const icl::Bf3Geom& g) {
  if (g.ksplit > 1) return 0;
  const int tiles_per = g.ntz * g.nty * g.ntx, per_xcd = (g.ntiles + 7) / 8;
  return g.nbatch == 1 || tiles_per % per_xcd == 0 ? g.wgs : 0;
}

// 3x3x3 forward / input gradient on the bf16 matrix pipe with every fp32 operand split exactly into three bf16 terms (six MFMA terms
// per product, fp32 accumulation: fp32 accuracy at 2.67x the fp32 matrix rate, kernels/conv_bf16x3.h).  Takes the same packed fp32
// weights as the fp32 kernels.  Not ok — left to them: Cin not a multiple of 16, rows not 16-byte granular, or a volume too small for
// its tiles to fill the chip.
SplitPlan plan_conv_split(const ConvShape& s, const ConvEnv& e) {
  SplitPlan p{};
  p.s = s;
  const int coutP = round_up(s.cout, 16), nchunks = s.cin / 16;
  const long vox = (long)s.d * s.h * s.w;
  // from 24^3 on (round 3, with schedule variant 60; batch 2, fp32 flat-tile kernel in brackets): 64->64 @24^3 62 us (78), 128->64 111
  // (125), 64->128 117 (137), 32->64 35 (50); at 12^3 the 4 x 8 x 16 tiles leave most of the chip idle: 128->128 108 us (44)
  // Round 6: rows of 12 voxels (the 12^3 level) on flat 4 x 4 x 12 tiles, split over the channel chunks so that the 18 tiles of a batch
  // of two fill the chip (kernels/conv_bf16x3.h Bf3F12); needs two cout blocks per workgroup (CoutP % 32 == 0) and the slab workspace.
  const bool f12_shape = s.w == icl::Bf3F12::TX && s.h % icl::Bf3F12::TY == 0 && s.d % icl::Bf3F12::TZ == 0 && coutP % 32 == 0 && e.flat12;
  // ... and a whole 6^3 volume (the centre block) as ONE flat tile (Bf3F6), likewise for split launches only
  const bool f6 = s.w == 6 && s.h == 6 && s.d == 6 && coutP % 32 == 0 && e.flat6;
  const long min_vox = e.min_vox ? atol(e.min_vox) : (f6 ? 216L : f12_shape ? 12L * 12 * 12 : 24L * 24 * 24);
  if (!e.split || (s.cin & 15) || ((s.w & 3) && !f6) || vox < min_vox || vox * 64 > (1L << 31)) return p;
  p.ok = true;
  p.w_bytes = (int64_t)nchunks * 3 * 6 * icl::Bf3::SLOTS * coutP * 16;
  // rows of 24 voxels: flat 2 x 8 x 24 tiles (kernels/conv_bf16x3.h Bf3F24) instead of 4 x 8 x 16 ones whose second x tile is half empty
  const bool f24 = s.w == icl::Bf3F24::TX && e.flat24, f12 = f12_shape && !f24;
  p.flat = f6 ? 6 : f12 ? 12 : (f24 ? 24 : 0);
  p.nbt = (f12 || f6) ? 2 : coutP % 48 == 0 ? 3 : (s.cout > 16 ? 2 : 1);
  // split over the channel chunks (flat tiles only): slices x dense output
  const double out_bytes = 4.0 * s.n * s.cout * vox;
  p.ksplit = 1;
  if (f6) p.ksplit = choose_ksplit_bf3((long)s.n * (coutP / 32), nchunks, e.cus, 8.0, out_bytes);      // one 8-wave workgroup per CU
  else if (f12) p.ksplit = choose_ksplit_bf3((long)s.n * (s.d / icl::Bf3F12::TZ) * (s.h / icl::Bf3F12::TY) * (coutP / 32), nchunks, 2 * e.cus, 6.0,
                                             out_bytes);      // two workgroups per CU
  else if (f24) p.ksplit = choose_ksplit_bf3((long)s.n * cdivl(s.d, icl::Bf3F24::TZ) * cdivl(s.h, icl::Bf3F24::TY) * cdivl(coutP, 16 * p.nbt), nchunks,
                                             e.cus, 6.0 * p.nbt, out_bytes);
  if (e.ksplit >= 0) p.ksplit = e.ksplit == 0 ? 1 : (e.ksplit < nchunks ? e.ksplit : nchunks);
  if (p.ksplit < 1) p.ksplit = 1;
  p.slab_bytes = p.ksplit > 1 ? (int64_t)p.ksplit * s.n * s.cout * vox * 4 : 0;
  p.g = split_geom(s, p.flat, p.ksplit);
  p.slots = split_stats_slots(p.g);
  return p;
}

// Runs a split-product plan; 1: not this kernel, the fp32 kernels take the call.  a.wp == nullptr: ws holds the split weights already
// (the pre-split entry points); else they are split into ws, and the slab of a split launch lies behind them (icl_conv3d_fwd_ws_bytes).
// slab: the workspace of the split launches of the pre-split entry points (icl_conv3d_fwd_presplit_ws).  No slab, no split.
// stats != nullptr: the epilogue writes the InstanceNorm statistics of the output there.
int conv_fwd_split_launch(const SplitPlan& p, const ConvArgs& a, float* ws, float* stats = nullptr, float* slab = nullptr) {
  if (!p.ok || (a.ybs & 3) || !ws || !aligned16(ws) || !aligned16(a.y)) return 1;
  if (a.wp && p.ksplit > 1) slab = ws + p.w_bytes / 4;
  const int ksplit = slab ? p.ksplit : 1;
  // the 12-voxel rows and the 6^3 tile exist for split launches only: without a workspace, or with one chunk, the fp32 kernels take the call
  if ((p.flat == 12 || p.flat == 6) && ksplit <= 1) return 1;
  icl::Bf3Geom g = ksplit == p.ksplit ? p.g : split_geom(p.s, p.flat, 1);      // (rows of 24 without a slab: the unsplit launch)
  g.x_bstride = a.xbs; g.y_bstride = a.ybs;
  if (ksplit > 1) g.slab = slab;
  if (stats) {
    if (!split_stats_slots(g)) return 1;
    g.stats = stats;
  }
  if (p.nbt == 2) return conv_fwd_split_go<2>(a.x, a.wp, a.bias, a.y, (uint4*)ws, g, a.stream, p.flat);
  if (p.nbt == 3) return conv_fwd_split_go<3>(a.x, a.wp, a.bias, a.y, (uint4*)ws, g, a.stream, p.flat);
  return conv_fwd_split_go<1>(a.x, a.wp, a.bias, a.y, (uint4*)ws, g, a.stream, p.flat);
}

template <int KS>
int conv_fwd_launch(const ConvShape& s, const ConvArgs& a, float* ws) {
  const ConvEnv e = conv_env();
  if (KS == 3) {
    const int rc = conv_fwd_split_launch(plan_conv_split(s, e), a, ws);
    if (rc != 1) return rc;
  }
  const Fp32Plan p = plan_conv_fp32<KS>(s, e);
  return p.rc ? p.rc : p.go(p, a, ws);
}

template <int KS, bool VEC>
int conv_wgrad_dispatch(const float* x, const float* gy, float* gwp, const icl::ConvGeom& g, dim3 grid, size_t lds, int mtp,
                        hipStream_t stream) {
  constexpr int T = KS * KS * KS;
  constexpr int NTW = (T + kConvWaves - 1) / kConvWaves;
  if (lds > (size_t)kMaxDynLds) ICL_SET_MAX_DYN_LDS((icl::conv3d_mfma_wgrad_kernel<KS, NTW, kConvWaves, VEC>), kMaxDynLdsBig);
  ICL_LAUNCH((icl::conv3d_mfma_wgrad_kernel<KS, NTW, kConvWaves, VEC>), grid, dim3(kConvWaves * 64), lds, stream, x, gy, gwp, g, mtp);
  snprintf(g_kernel, sizeof(g_kernel), "conv3d_mfma_wgrad_kernel<%d, %d, 4, %s>", KS, (KS * KS * KS + 3) / 4, VEC ? "true" : "false");
  return check_launch("conv3d_wgrad");
}

template <int KS>
int conv_wgrad_launch(const float* x, const float* gy, float* gwp, int n, int n_live, int cin, int cout, int d, int h, int w,
                      int64_t xbs, int64_t gbs, int* nslabs, hipStream_t stream) {
  icl::ConvGeom g = conv_geom(cin, cout, d, h, w, xbs, gbs);
  if (KS == 3) {
    const int rc = conv_wgrad_static(x, gy, gwp, g, n, n_live, nslabs, stream);
    if (rc != 1) return rc;
  }
  const bool vec = (w % 4) == 0;
  choose_tile(g, KS, 256, vec);
  g.KC = 16;
  g.CPP = 4;
  g.ksplit = 1;
  // staging-table limit: CPP * PZ * PY * Q items per pass must fit kJX per thread
  for (;;) {
    const int per_ch = (g.TZ + KS - 1) * (g.TY + KS - 1) * (g.PXL / (vec ? 4 : 1));
    if (g.CPP * per_ch <= icl::kJX * kConvWaves * 64) break;
    if (g.TZ > 1) g.TZ = largest_divisor_le(g.D, g.TZ - 1);
    else if (g.TY > 1) g.TY = largest_divisor_le(g.H, g.TY - 1);
    else return fail(-1, "conv3d_wgrad: row too wide to stage");
  }
  if (vec) finish_tile(g, KS, 4, 8); else finish_tile(g, KS, 2, 32);
  const int mt = g.TZ * g.TY * g.TX;
  if (mt > 256) return fail(-1, "conv3d_wgrad: tile of %d voxels too large", mt);
  int mtp = mt;
  while (mtp % 32 != 2) ++mtp;
  const size_t lds = (size_t)16 * (g.PS + mtp) * 4;
  if (lds > (size_t)kMaxDynLdsBig) return fail(-1, "conv3d_wgrad: LDS tile %zu B too large", lds);
  const int pairs = (g.CoutP / 16) * ((g.CinP + 15) / 16);
  const int ntiles = g.ntx * g.nty * g.ntz;
  int nsplit = wgrad_max_split(pairs, n);
  if (nsplit > ntiles) nsplit = ntiles;
  *nslabs = nsplit * n * (KS == 1 ? kConvWaves : 1);
  dim3 grid(nsplit, pairs, n);
  return vec ? conv_wgrad_dispatch<KS, true>(x, gy, gwp, g, grid, lds, mtp, stream)
             : conv_wgrad_dispatch<KS, false>(x, gy, gwp, g, grid, lds, mtp, stream);
}

}  // namespace

// ---- Swin window attention ---------------------------------------------------------------------------------------

static int winattn_geom(icl::WinAttnGeom& g, int b_, int n, int heads, int nw, int dh, float scale, const char* who) {
  if (b_ < 1 || n < 1 || n > 352 || heads < 1 || nw < 1 || b_ % nw != 0) return fail(-1, "%s: bad argument (1 <= n <= 352, B_ %% nW == 0)", who);
  if (dh != 16 && !(dh == 32 && n <= 96)) return fail(-1, "%s: head dim 16 (n <= 352) or 32 (n <= 96) supported, got %d with n = %d", who, dh, n);
  g.B_ = b_; g.n = n; g.npad = (n + 15) / 16 * 16; g.heads = heads; g.nW = nw; g.scale = scale;
  return 0;
}

int64_t icl_window_attn_bias_elems_impl(int n, int heads) { return (int64_t)heads * n * ((n + 15) / 16 * 16); }

// The launchers take the kernels' optional trailing argument (const icl::WaDrop&, attention dropout) as a pack and hand it on: with the
// pack empty they launch the p = 0 instantiations, with it the dropout ones — one kernel choice, one set of LDS sizes for both.
template <int NKB, int DH, typename... DR>
static int winattn_fwd_launch(const float* qkv, const float* bias, const int* regions, float* out, float* lse, const icl::WinAttnGeom& g,
                              hipStream_t st, const DR&... dr) {
  const size_t lds = ((size_t)2 * g.npad * icl::WaCfg<DH>::LD + g.npad) * 4;
  if (g.npad == NKB * 16) {
    ICL_LAUNCH((icl::window_attn_fwd_kernel<NKB, DH, true>), dim3((unsigned)g.B_ * g.heads), dim3(icl::kWaThreads), lds, st, qkv, bias, regions, out, lse, g, dr...);
  } else {
    ICL_LAUNCH((icl::window_attn_fwd_kernel<NKB, DH, false>), dim3((unsigned)g.B_ * g.heads), dim3(icl::kWaThreads), lds, st, qkv, bias, regions, out, lse, g, dr...);
  }
  snprintf(g_kernel, sizeof(g_kernel), "window_attn_fwd_kernel<%d, %d%s>", NKB, DH, sizeof...(DR) ? ", WaDrop" : "");
  return check_launch("window_attn_fwd");
}

// window slices of the dQ / d(bias) kernel: enough to fill the chip (two workgroups per CU), at least ~4 windows per slice so that the
// bias slabs (one per slice, summed by relpos_bias_gather_sum_kernel) stay small
static int winattn_bias_chunks(const icl::WinAttnGeom& g) {
  const int nkb = g.npad / 16, gx = (nkb + icl::kWaWaves - 1) / icl::kWaWaves;
  int chunks = (512 + gx * g.heads - 1) / (gx * g.heads);
  if (chunks > (g.B_ + 3) / 4) chunks = (g.B_ + 3) / 4;
  return chunks < 1 ? 1 : chunks;
}

template <int NKB, int DH, typename... DR>
static int winattn_q_bias_launch(const float* qkv, const float* bias, const int* regions, const float* out, const float* lse,
                                 const float* dout, float* dqkv, float* dbias, const icl::WinAttnGeom& g, hipStream_t st, const DR&... dr) {
  const size_t lds = ((size_t)2 * g.npad * icl::WaCfg<DH>::LD + g.npad) * 4;
  const int nkb = g.npad / 16, gx = (nkb + icl::kWaWaves - 1) / icl::kWaWaves;
  const int chunks = winattn_bias_chunks(g);
  if (g.npad == NKB * 16) {
    ICL_LAUNCH((icl::window_attn_bwd_q_bias_kernel<NKB, DH, true>), dim3(gx, g.heads, chunks), dim3(icl::kWaThreads), lds, st, qkv, bias,
               regions, out, lse, dout, dqkv, dbias, g, dr...);
  } else {
    ICL_LAUNCH((icl::window_attn_bwd_q_bias_kernel<NKB, DH, false>), dim3(gx, g.heads, chunks), dim3(icl::kWaThreads), lds, st, qkv, bias,
               regions, out, lse, dout, dqkv, dbias, g, dr...);
  }
  return check_launch("window_attn_bwd_q_bias");
}

template <int DH, typename... DR>
static int winattn_kv_launch(const float* qkv, const float* bias, const int* regions, const float* out, const float* lse,
                             const float* dout, float* dqkv, const icl::WinAttnGeom& g, hipStream_t st, const DR&... dr) {
  const size_t lds = ((size_t)2 * g.npad * icl::WaCfg<DH>::LD + 3 * g.npad) * 4;
  ICL_LAUNCH((icl::window_attn_bwd_kv_kernel<DH>), dim3((unsigned)g.B_ * g.heads), dim3(icl::kWaThreads), lds, st, qkv, bias, regions, out,
             lse, dout, dqkv, g, dr...);
  return check_launch("window_attn_bwd_kv");
}

// the forward of icl_window_attn_fwd and icl_window_attn_fwd_drop: which kernel, for p = 0 and for dropout alike
template <typename... DR>
static int winattn_fwd_dispatch(const float* qkv, const float* bias, const int* regions, float* out, float* lse, const icl::WinAttnGeom& g,
                                int head_dim, hipStream_t st, const DR&... dr) {
  const int nkb = g.npad / 16;
  // ICL_WINATTN_ONLINE (default 1): online softmax over chunks of four key blocks, four waves per SIMD (kernels/winattn.h), for the
  // 343- / 216-token windows of SwinUNETR; 0: the whole score row block of a wave in registers
  const char* e_on = getenv("ICL_WINATTN_ONLINE");
  // (measured, batch 2: 686 windows x 3 heads 420 -> 354 us, 128 x 6 heads 137 -> 122; with 192 workgroups or fewer the chip is not
  // full either way and the extra rescaling costs 7 %: those stay on the register-resident form)
  const int online = e_on ? atoi(e_on) : 1;             // 2: whatever the size (tests)
  if (head_dim == 16 && ((nkb > 6 && (long)g.B_ * g.heads >= 512 && online == 1) || online == 2)) {
    const size_t lds = ((size_t)2 * g.npad * (16 + 4) + g.npad) * 4;
    ICL_SET_MAX_DYN_LDS((icl::window_attn_fwd_online_kernel<16, DR...>), 64 * 1024);
    ICL_LAUNCH((icl::window_attn_fwd_online_kernel<16>), dim3((unsigned)g.B_ * g.heads), dim3(icl::kWaThreads), lds, st, qkv, bias, regions,
               out, lse, g, dr...);
    snprintf(g_kernel, sizeof(g_kernel), "window_attn_fwd_online_kernel<16%s>", sizeof...(DR) ? ", WaDrop" : "");
    return check_launch("window_attn_fwd_online");
  }
  if (head_dim == 32) return winattn_fwd_launch<6, 32>(qkv, bias, regions, out, lse, g, st, dr...);
  if (nkb > 14) return winattn_fwd_launch<22, 16>(qkv, bias, regions, out, lse, g, st, dr...);
  if (nkb > 6) return winattn_fwd_launch<14, 16>(qkv, bias, regions, out, lse, g, st, dr...);
  return winattn_fwd_launch<6, 16>(qkv, bias, regions, out, lse, g, st, dr...);
}

template <typename... DR>
static int winattn_bwd_dispatch(const float* qkv, const float* bias, const int* regions, const float* out, const float* lse,
                                const float* dout, float* dqkv, float* dbias, const icl::WinAttnGeom& g, int head_dim, hipStream_t st,
                                const DR&... dr) {
  if (int rc = head_dim == 32 ? winattn_kv_launch<32>(qkv, bias, regions, out, lse, dout, dqkv, g, st, dr...)
                              : winattn_kv_launch<16>(qkv, bias, regions, out, lse, dout, dqkv, g, st, dr...))
    return rc;
  const int nkb = g.npad / 16;      // (dbias: icl_window_attn_bwd_chunks(...) slabs, every used element written: no memset)
  if (head_dim == 32) return winattn_q_bias_launch<6, 32>(qkv, bias, regions, out, lse, dout, dqkv, dbias, g, st, dr...);
  if (nkb > 14) return winattn_q_bias_launch<22, 16>(qkv, bias, regions, out, lse, dout, dqkv, dbias, g, st, dr...);
  if (nkb > 6) return winattn_q_bias_launch<14, 16>(qkv, bias, regions, out, lse, dout, dqkv, dbias, g, st, dr...);
  return winattn_q_bias_launch<6, 16>(qkv, bias, regions, out, lse, dout, dqkv, dbias, g, st, dr...);
}

// Attention dropout: seed / threshold / scale of one launch (the mask is regenerated from (seed, index) in every kernel).
static int winattn_drop_spec(icl::WaDrop& d, uint32_t seed, float p, const uint32_t* seed_dev, const char* who) {
  if (!(p > 0.f && p < 1.f)) return fail(-1, "%s: 0 < p < 1 required (p = 0 is the kernel without dropout)", who);
  d.seed = (unsigned)seed;
  d.thresh = (unsigned)((double)p * 4294967296.0);      // as icl_drop_path_add
  d.scale = 1.f / (1.f - p);
  d.seed_dev = (const unsigned*)seed_dev;
  return 0;
}

// ---- dense products (kernels/gemm.h) ------------------------------------------------------------------------------
namespace {

struct GemmPlan { int wm, wn, nsplit, kper, kt, tn; };

// Block shape by the output's aspect; split-K when the grid would leave most of the 256 CUs idle.
GemmPlan gemm_plan(long M, int N, int K, int batch, bool narrow_ok = false) {
  GemmPlan p;
  p.tn = 4;
  if (N <= 64) { p.wm = 4; p.wn = 1; }
  else if (M <= 64) { p.wm = 1; p.wn = 4; }
  else { p.wm = 2; p.wn = 2; }
  if (narrow_ok && M > 64 && N % 48 == 0 && N % 64 != 0 && N <= 576) {
    // Linear layers of the Swin stages (48 / 96 / 144 / 288 ... outputs): 48-column wave tiles, no padded columns
    p.tn = 3;
    if (N % 144 == 0) { p.wm = 2; p.wn = 3; }       // 128 x 144 block, six waves
    else if (N % 96 == 0) { p.wm = 2; p.wn = 2; }   // 128 x 96
    else { p.wm = 4; p.wn = 1; }                    // 256 x 48
  }
  constexpr int force = 0;   // tuning knob
  const long blocks = cdivl(M, p.wm * 64) * cdivl(N, p.wn * 16 * p.tn) * batch;
  const int ksteps = (K + 31) / 32;
  int ns = 1;
  if (force > 0) ns = force;
  else if (blocks <= 384 && ksteps >= 8) {
    // all workgroups of the launch resident at once: 3 per CU (register-limited) x 256 CUs = 768 slots.  A grid of 864 ran as
    // 768 + a second round of 96 on a mostly idle chip (PMC: 1.6 resident waves per SIMD on average, 92 instead of 104 TFLOP/s).
    ns = (int)(768 / blocks);
    if (ns > ksteps / 4) ns = ksteps / 4;           // at least 4 k-steps (128 deep) per split
  }
  // (measured and dropped, round 4: one k-step per workgroup + the slab sum for products of one or two workgroups — the 216^2 token-axis MLP of
  // the 6^3 level runs 33 us in ONE workgroup — 11.71 / 11.80 against 11.84 / 11.72 ms per step: that chain is not what the step waits for)
  if (ns > ksteps) ns = ksteps;
  if (ns < 1) ns = 1;
  const int per = (ksteps + ns - 1) / ns;
  p.kper = per * 32;
  p.nsplit = (ksteps + per - 1) / per;
  p.kt = 32;      // 64-deep steps (64 KiB LDS, two workgroups per CU) were measured slower on every shape
  return p;
}

template <bool AK, bool BK_, bool FAST>
int gemm_launch_cfg(icl::GemmArgs g, const GemmPlan& p, int batch, hipStream_t st) {
  dim3 grid((unsigned)cdivl(g.N, p.wn * 16 * p.tn), (unsigned)cdivl(g.M, p.wm * 64), (unsigned)(batch * p.nsplit));
  // (~n resident workgroups walking the row blocks of a tall product instead of one short-lived workgroup per block: measured on the
  // Swin stage-0 Linear layers, 221,184 rows, K = 48..192 — no gain at 512 / 768 / 1024 workgroups; the kernel keeps its loop over
  // gridDim.y-strided row blocks, the launcher always gives every block its own workgroup)
  size_t lds = (size_t)(p.wm * 64 + p.wn * 16 * p.tn) * 32 * 4;
  const size_t ep = (size_t)p.wm * p.wn * 32 * (16 * p.tn + 4) * 4;     // store transposition buffer of the k-contiguous-B epilogue
  if (BK_ && ep > lds) lds = ep;
  if constexpr (AK && BK_ && FAST) {
    if (p.tn == 3) {
      if (p.wn == 3) ICL_LAUNCH((icl::gemm_kernel<true, true, 2, 3, true, 32, 3>), grid, dim3(384), lds, st, g);
      else if (p.wn == 2) ICL_LAUNCH((icl::gemm_kernel<true, true, 2, 2, true, 32, 3>), grid, dim3(256), lds, st, g);
      else ICL_LAUNCH((icl::gemm_kernel<true, true, 4, 1, true, 32, 3>), grid, dim3(256), lds, st, g);
      return check_launch("gemm");
    }
  }
  if (p.wm == 4) ICL_LAUNCH((icl::gemm_kernel<AK, BK_, 4, 1, FAST>), grid, dim3(256), lds, st, g);
  else if (p.wm == 1) ICL_LAUNCH((icl::gemm_kernel<AK, BK_, 1, 4, FAST>), grid, dim3(256), lds, st, g);
  else ICL_LAUNCH((icl::gemm_kernel<AK, BK_, 2, 2, FAST>), grid, dim3(256), lds, st, g);
  return check_launch("gemm");
}

// 16-byte staging loads need aligned bases / pitches, K % 4 == 0 for a k-contiguous operand, rows % 4 == 0 for a k-strided one
inline bool gemm_operand_fast(const float* p, long ld, long bstride, bool kcontig, long rows, int K) {
  return aligned16(p) && (ld & 3) == 0 && (bstride & 3) == 0 && (kcontig ? (K & 3) == 0 : ((rows & 3) == 0 && rows >= 4));
}

int64_t gemm_ws_bytes_impl(long M, int N, int K, int batch) {
  // the run-time plan depends on operand alignment (48-column tiles need the 16-byte staging path): size for either
  int ns = 1;
  for (int narrow = 0; narrow < 2; ++narrow) {
    const GemmPlan p = gemm_plan(M, N, K, batch, narrow != 0);
    if (p.nsplit > ns) ns = p.nsplit;
  }
  return (ns > 1 || batch > 1) ? (int64_t)ns * batch * M * N * 4 : 0;   // batch > 1: the caller may ask for the batch sum
}

// C[b] = act(A[b] B[b] + bias); ws holds the split-K slabs ([split][batch][M][N]) when the plan splits.
// batch > 1 with c_bs == 0: C = act(sum_b A[b] B[b] + bias) — the batch entries are summed like split-K partials.
int gemm_run(const float* a, const float* b, float* c, const float* bias, void* ws, long M, int N, int K, long lda, long ldb, long ldc,
             int a_kcontig, int b_kcontig, int act, int batch, long a_bs, long b_bs, long c_bs, hipStream_t st) {
  const bool fast = gemm_operand_fast(a, lda, a_bs, a_kcontig != 0, M, K) && gemm_operand_fast(b, ldb, b_bs, b_kcontig != 0, N, K);
  GemmPlan p = gemm_plan(M, N, K, batch, fast && a_kcontig && b_kcontig);
  const bool sum_batch = batch > 1 && c_bs == 0;
  constexpr int trace = 0;
  if (trace)
    fprintf(stderr, "[icl gemm] M %ld N %d K %d batch %d  a_k %d b_k %d fast %d  tile %dx%d waves, split %d (k per split %d)%s\n", M, N, K, batch,
            a_kcontig, b_kcontig, (int)fast, p.wm, p.wn, p.nsplit, p.kper, ws ? "" : "  no workspace");
  if (sum_batch && ((N & 3) || (ldc & 3) || !ws)) return fail(-1, "gemm: a batch sum needs the workspace, N %% 4 == 0 and ldc %% 4 == 0");
  if (p.nsplit > 1 && ((N & 3) || (ldc & 3) || !ws)) {   // the slab reduction works on 16-byte pieces: run unsplit
    p.nsplit = 1;
    p.kper = (K + 31) / 32 * 32;
  }
  icl::GemmArgs g{};
  g.a = a; g.b = b; g.bias = bias;
  g.lda = lda; g.ldb = ldb;
  g.a_bstride = a_bs; g.b_bstride = b_bs;
  g.M = (int)M; g.N = N; g.K = K; g.kper = p.kper; g.nsplit = p.nsplit; g.act = act;
  const bool split = p.nsplit > 1 || sum_batch;
  if (split) {
    g.c = (float*)ws; g.ldc = N; g.c_bstride = M * N; g.c_split_stride = (long)batch * M * N;
  } else {
    g.c = c; g.ldc = ldc; g.c_bstride = c_bs; g.c_split_stride = 0;
  }
  int rc;
  if (fast) {
    if (a_kcontig) rc = b_kcontig ? gemm_launch_cfg<true, true, true>(g, p, batch, st) : gemm_launch_cfg<true, false, true>(g, p, batch, st);
    else rc = b_kcontig ? gemm_launch_cfg<false, true, true>(g, p, batch, st) : gemm_launch_cfg<false, false, true>(g, p, batch, st);
  } else {
    if (a_kcontig) rc = b_kcontig ? gemm_launch_cfg<true, true, false>(g, p, batch, st) : gemm_launch_cfg<true, false, false>(g, p, batch, st);
    else rc = b_kcontig ? gemm_launch_cfg<false, true, false>(g, p, batch, st) : gemm_launch_cfg<false, false, false>(g, p, batch, st);
  }
  if (rc || !split) return rc;
  if (sum_batch) {
    ICL_LAUNCH(icl::gemm_reduce_slabs_kernel, dim3(grid_for(M * (N / 4), 256, 2048)), dim3(256), 0, st, (const float*)ws, c, bias,
               p.nsplit * batch, M, N, (long)N, M * N, ldc, act);
    return check_launch("gemm_reduce");
  }
  for (int bi = 0; bi < batch; ++bi) {
    ICL_LAUNCH(icl::gemm_reduce_slabs_kernel, dim3(grid_for(M * (N / 4), 256, 2048)), dim3(256), 0, st, (const float*)ws + (long)bi * M * N,
               c + bi * c_bs, bias, p.nsplit, M, N, (long)N, (long)batch * M * N, ldc, act);
    if ((rc = check_launch("gemm_reduce"))) return rc;
  }
  return 0;
}

// the weight-streaming kernels take every input of <= 32 rows: HBM-bound on the 13,824^2 matrices, and for the small Linear layers
// of the aligner (4..32 rows) a 16-row MFMA tile per wave instead of the 64-row tiles of the general product
inline bool linear_streams(long rows, int in, int out) {
  constexpr int on = 1;
  return on && rows <= 32 && (in & 3) == 0 && (out & 3) == 0;
}
struct StreamPlan { int mt, nslice, slice_len, upw, groups; };

// One workgroup per CU (8 waves, the slice of the small operand resident in LDS): slices x unit groups ~ 256 workgroups.
StreamPlan stream_plan(long rows, int in, int out, bool nn) {
  StreamPlan p;
  p.mt = rows <= 16 ? 1 : 2;
  const int cdim = nn ? out : in;
  const int units = nn ? (in + 63) / 64 : (out + 15) / 16;
  // tuning knob.  Round 4: 1536 -> 1024 (64 KiB of LDS for the slice, 96 KiB per workgroup): 11.33 -> 11.16 ms per step (768: 11.25, 512: 11.45;
  // profiles/r4_schedule_experiments.txt [r4_sd*.txt]) — the streams' workgroups leave LDS for the small kernels that run beside them
  constexpr int maxcols = 1024;
  const int maxlen = maxcols / p.mt;
  int nslice = (cdim + maxlen - 1) / maxlen;
  const int groups1 = (units + 7) / 8;
  const bool big = (long)in * out >= (1L << 20);
  for (;;) {
    p.slice_len = ((cdim + nslice - 1) / nslice + 63) / 64 * 64;
    p.nslice = (cdim + p.slice_len - 1) / p.slice_len;
    // mid-size matrices (1,728^2): more, shorter slices until the chip is half full.  Small ones stay one slice (no slab sum
    // launch) unless fewer than 16 workgroups would stream them (1024 x 256 input gradient: 4 column strips = ONE workgroup, 42 us).
    const long wgs = (long)p.nslice * groups1;
    // (small matrices: a second slice costs a slab-sum launch, ~8 us with its boundary — worth it only while fewer than
    // `small_min` workgroups would stream the weights; measured in the step: 16 -> 8)
    constexpr int small_min = 8;
    if (big ? (wgs * 4 <= 256 && p.slice_len >= 512) : (wgs < small_min && p.slice_len >= 128)) nslice = p.nslice * 2;
    else break;
  }
  const int gt = 256 / p.nslice > 0 ? 256 / p.nslice : 1;
  p.upw = (units + 8 * gt - 1) / (8 * gt);
  p.groups = (units + 8 * p.upw - 1) / (8 * p.upw);
  return p;
}

template <int MT, bool NN>
int stream_launch(const float* xs, const float* w, float* slab, int M, int K, int O, const StreamPlan& p, const float* bias, int act,
                  hipStream_t st, const float* wg_x = nullptr, float* wg_dw = nullptr) {
  // wg_dw: extra workgroup columns compute the weight gradient in the same launch (kernels/gemm.h)
  const int wg_blocks = wg_dw ? grid_for((long)O * (K / 4), 512, 2048) : 0;
  const dim3 grid(p.groups + wg_blocks, p.nslice);
  const size_t lds = ((size_t)16 * MT * p.slice_len + 8 * 1024) * 4;
  // four 16 x 64 weight tiles in flight per wave (128 KB per CU; six measured the same and were removed in round 5)
  ICL_SET_MAX_DYN_LDS((icl::linear_stream_kernel<MT, NN, 4>), 160 * 1024);
  ICL_LAUNCH((icl::linear_stream_kernel<MT, NN, 4>), grid, dim3(512), lds, st, xs, w, slab, M, K, O, p.slice_len, p.upw, bias, act, wg_x, wg_dw, wg_blocks);
  return check_launch("linear_stream");
}

// y / gx = act(bias + sum over slices): the streaming kernel followed by the fixed-order slab sum
int stream_run(const float* xs, const float* w, const float* bias, float* y, void* ws, long rows, int in, int out, bool nn, int act,
               hipStream_t st, const float* wg_x = nullptr, float* wg_dw = nullptr) {
  const StreamPlan p = stream_plan(rows, in, out, nn);
  const bool direct = p.nslice == 1;                      // single slice: the kernel writes y itself (bias, activation included)
  float* slab = direct ? y : (float*)ws;
  if (!slab) return fail(-1, "linear: the streaming plan needs the workspace of icl_linear_ws_bytes()");
  const int M = (int)rows;
  // several slices: gemm_reduce_slabs_kernel adds the slices' partials in slice order (a second, small launch: summing them in the
  // last-arriving workgroup instead was built in round 4, bit-identical, and measured slower — the hand-over needs whole-L2 write-back /
  // invalidate on gfx950; profiles/r4_tickets_ab.txt; removed in round 5)
  int rc;
  if (p.mt == 1) rc = nn ? stream_launch<1, true>(xs, w, slab, M, in, out, p, bias, act, st, wg_x, wg_dw) : stream_launch<1, false>(xs, w, slab, M, in, out, p, bias, act, st);
  else rc = nn ? stream_launch<2, true>(xs, w, slab, M, in, out, p, bias, act, st, wg_x, wg_dw) : stream_launch<2, false>(xs, w, slab, M, in, out, p, bias, act, st);
  if (rc || direct) return rc;
  const int n = nn ? in : out;
  ICL_LAUNCH(icl::gemm_reduce_slabs_kernel, dim3(grid_for(rows * (n / 4), 256, 1024)), dim3(256), 0, st, (const float*)slab, y, bias, p.nslice,
             rows, n, (long)n, (long)16 * p.mt * n, (long)n, act);
  return check_launch("linear_stream_reduce");
}

inline int64_t stream_ws_bytes(long rows, int in, int out, bool nn) {
  const StreamPlan p = stream_plan(rows, in, out, nn);
  return p.nslice == 1 ? 0 : (int64_t)p.nslice * 16 * p.mt * (nn ? in : out) * 4;
}

}  // namespace

namespace {
// tall, skinny Linear with the weights held in registers (kernels/gemm.h linear_rows_kernel): the token layers of SwinUNETR stage 0.
// Returns 1 when the shape has no instantiation (K, N multiples of 16 with N K <= 9216) or the call is small / misaligned.
template <int KQ, int NT, bool WT>
int linear_rows_go(const float* x, const float* w, const float* bias, float* y, long rows, int act, hipStream_t st) {
  constexpr int NH = NT >= 9 ? 3 : 1;                     // 144 / 192 columns: three waves share a row block (48 / 64 columns each)
  const size_t lds = (size_t)4 * 16 * (16 * NT / NH + 4) * 4;
  long blocks = (rows + 63) / 64 * NH;
  if (blocks > 2040) blocks = 2040;                      // ~8 workgroups per CU (a multiple of 3), each wave walks its share of the row blocks
  blocks = (blocks + NH - 1) / NH * NH;
  ICL_LAUNCH((icl::linear_rows_kernel<KQ, NT, WT, NH>), dim3((unsigned)blocks), dim3(256), lds, st, x, w, bias, y, rows, act);
  snprintf(g_kernel, sizeof(g_kernel), "linear_rows_kernel<%d, %d, %s>", KQ, NT, WT ? "true" : "false");
  return check_launch("linear_rows");
}

template <bool WT>
int linear_rows(const float* x, const float* w, const float* bias, float* y, long rows, int k, int n, int act, hipStream_t st) {
  constexpr int on = 1;
  if (!on || rows < 16384 || (act != 0 && act != 1) || !aligned16(x) || !aligned16(w) || !aligned16(y)) return 1;
#define ICL_ROWS_CASE(KK, NN) if (k == KK && n == NN) return linear_rows_go<KK / 16, NN / 16, WT>(x, w, bias, y, rows, act, st);
  ICL_ROWS_CASE(48, 48) ICL_ROWS_CASE(48, 144) ICL_ROWS_CASE(48, 192) ICL_ROWS_CASE(192, 48) ICL_ROWS_CASE(144, 48)
  ICL_ROWS_CASE(96, 96) ICL_ROWS_CASE(48, 96) ICL_ROWS_CASE(96, 48)
#undef ICL_ROWS_CASE
  return 1;
}
}  // namespace

extern "C" {

int icl_abi_version(void) { return 1; }
const char* icl_last_error(void) { return g_err; }
const char* icl_last_kernel_name(void) { return g_kernel; }
const char* icl_last_resample_route(void) { return g_resample; }

int64_t icl_conv3d_packed_elems(int cout, int cin, int ks, int mode) {
  const int k = mode ? cout : cin, nn = mode ? cin : cout;
  return (int64_t)ks * ks * ks * round_up(k, 4) * round_up(nn, 16);
}

int icl_conv3d_pack_weights(const float* w, float* wp, int cout, int cin, int ks, int mode, void* stream) {
  if (!w || !wp || (ks != 1 && ks != 3) || cout < 1 || cin < 1) return fail(-1, "pack_weights: bad argument");
  const int T = ks * ks * ks;
  const int kp = round_up(mode ? cout : cin, 4), np = round_up(mode ? cin : cout, 16);
  const long total = (long)T * kp * np;
  ICL_LAUNCH(icl::pack_weights_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, w, wp, cout, cin, T, kp, np, mode);
  return check_launch("pack_weights");
}

int icl_conv3d_pack_weights_both(const float* w, float* wp_fwd, float* wp_dgrad, int cout, int cin, int ks, void* stream) {
  if (!w || !wp_fwd || !wp_dgrad || (ks != 1 && ks != 3) || cout < 1 || cin < 1) return fail(-1, "pack_weights_both: bad argument");
  const int T = ks * ks * ks;
  const int kp0 = round_up(cin, 4), np0 = round_up(cout, 16), kp1 = round_up(cout, 4), np1 = round_up(cin, 16);
  const long total = (long)T * kp0 * np0 + (long)T * kp1 * np1;
  ICL_LAUNCH(icl::pack_weights_both_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, w, wp_fwd, wp_dgrad, cout, cin, T,
             kp0, np0, kp1, np1);
  return check_launch("pack_weights_both");
}

int64_t icl_conv3d_split_ws_bytes(int cin, int cout) {
  if (cin < 16 || (cin & 15) || cout < 1) return 0;
  return (int64_t)(cin / 16) * 3 * 6 * icl::Bf3::SLOTS * round_up(cout, 16) * 16;
}

int icl_conv3d_split_weights_multi(const void* const* wp, void* const* wsplit, const int32_t* cin, const int32_t* cout, int count,
                                   void* stream) {
  if (!wp || !wsplit || !cin || !cout || count < 1) return fail(-1, "split_weights_multi: bad argument");
  for (int base = 0; base < count; base += icl::kSplitMulti) {
    icl::SplitMulti m{};
    const int k = count - base < icl::kSplitMulti ? count - base : icl::kSplitMulti;
    long tmax = 1;
    for (int i = 0; i < k; ++i) {
      const int j = base + i;
      if (!wp[j] || !wsplit[j] || cin[j] < 16 || (cin[j] & 15) || cout[j] < 1 || !aligned16(wsplit[j]))
        return fail(-1, "split_weights_multi: bad tensor %d (Cin must be a multiple of 16)", j);
      m.wp[i] = (const float*)wp[j]; m.ws[i] = (uint4*)wsplit[j];
      m.cinP[i] = round_up(cin[j], 4); m.coutP[i] = round_up(cout[j], 16); m.nchunks[i] = cin[j] / 16;
      const long t = (long)m.nchunks[i] * 3 * 2 * icl::Bf3::SLOTS * m.coutP[i];
      if (t > tmax) tmax = t;
    }
    ICL_LAUNCH(icl::conv_bf16x3_split_weights_multi_kernel, dim3(grid_for(tmax, 256, 1024), k), dim3(256), 0, (hipStream_t)stream, m);
    const int rc = check_launch("split_weights_multi");
    if (rc) return rc;
  }
  return 0;
}

// the pre-split entry points: wsplit holds the split weights already
static int presplit_launch(const float* x, const void* wsplit, const float* bias, float* y, float* stats, float* slab, int n, int cin, int cout,
                           int d, int h, int w, int64_t xbs, int64_t ybs, void* stream) {
  return conv_fwd_split_launch(plan_conv_split({n, cin, cout, d, h, w}, conv_env()), {x, nullptr, bias, y, xbs, ybs, (hipStream_t)stream},
                               (float*)const_cast<void*>(wsplit), stats, slab);
}

int icl_conv3d_fwd_presplit(const float* x, const void* wsplit, const float* bias, float* y, int n, int cin, int cout, int d, int h, int w,
                            int64_t x_bstride, int64_t y_bstride, void* stream) {
  if (!x || !wsplit || !y || n < 1 || cin < 1 || cout < 1 || d < 1 || h < 1 || w < 1) return fail(-1, "conv3d_fwd_presplit: bad argument");
  return presplit_launch(x, wsplit, bias, y, nullptr, nullptr, n, cin, cout, d, h, w, x_bstride, y_bstride, stream);
}

int64_t icl_conv3d_fwd_presplit_ws_bytes(int n, int cin, int cout, int d, int h, int w) {
  if (n < 1 || cin < 1 || cout < 1 || d < 1 || h < 1 || w < 1) return 0;
  const SplitPlan p = plan_conv_split({n, cin, cout, d, h, w}, conv_env());
  return p.ok ? p.slab_bytes : 0;
}

int icl_conv3d_fwd_presplit_ws(const float* x, const void* wsplit, const float* bias, float* y, void* ws, int n, int cin, int cout, int d,
                               int h, int w, int64_t x_bstride, int64_t y_bstride, void* stream) {
  if (!x || !wsplit || !y || n < 1 || cin < 1 || cout < 1 || d < 1 || h < 1 || w < 1) return fail(-1, "conv3d_fwd_presplit_ws: bad argument");
  if (ws && !aligned16(ws)) return fail(-1, "conv3d_fwd_presplit_ws: workspace not 16-byte aligned");
  return presplit_launch(x, wsplit, bias, y, nullptr, (float*)ws, n, cin, cout, d, h, w, x_bstride, y_bstride, stream);
}

int icl_conv3d_fwd_stats_slots(int n, int cin, int cout, int d, int h, int w) {
  const SplitPlan p = plan_conv_split({n, cin, cout, d, h, w}, conv_env());
  return p.ok ? p.slots : 0;
}

int icl_conv3d_fwd_presplit_stats(const float* x, const void* wsplit, const float* bias, float* y, float* stats, int n, int cin, int cout,
                                  int d, int h, int w, int64_t x_bstride, int64_t y_bstride, void* stream) {
  if (!x || !wsplit || !y || !stats || n < 1 || cin < 1 || cout < 1) return fail(-1, "conv3d_fwd_presplit_stats: bad argument");
  return presplit_launch(x, wsplit, bias, y, stats, nullptr, n, cin, cout, d, h, w, x_bstride, y_bstride, stream);
}

int icl_conv3d_pack_weights_multi(const void* const* w, void* const* wp_fwd, void* const* wp_dgrad, const int32_t* cout, const int32_t* cin,
                                  const int32_t* ks, int count, void* stream) {
  if (!w || !wp_fwd || !wp_dgrad || !cout || !cin || !ks || count < 1) return fail(-1, "pack_weights_multi: bad argument");
  for (int base = 0; base < count; base += icl::kPackMulti) {
    icl::PackMulti m{};
    const int k = count - base < icl::kPackMulti ? count - base : icl::kPackMulti;
    long tmax = 1;      // most 16 x 16 tiles of a weight in this launch
    for (int i = 0; i < k; ++i) {
      const int j = base + i;
      if (!w[j] || !wp_fwd[j] || !wp_dgrad[j] || cout[j] < 1 || cin[j] < 1 || (ks[j] != 1 && ks[j] != 3))
        return fail(-1, "pack_weights_multi: bad tensor %d", j);
      m.w[i] = (const float*)w[j]; m.wp0[i] = (float*)wp_fwd[j]; m.wp1[i] = (float*)wp_dgrad[j];
      m.cout[i] = cout[j]; m.cin[i] = cin[j]; m.taps[i] = ks[j] * ks[j] * ks[j];
      const long t = (long)(round_up(cout[j], 16) / 16) * (round_up(cin[j], 16) / 16);
      if (t > tmax) tmax = t;
    }
    ICL_LAUNCH(icl::pack_weights_multi_kernel, dim3((unsigned)(tmax < 1024 ? tmax : 1024), k), dim3(256), 0, (hipStream_t)stream, m);
    const int rc = check_launch("pack_weights_multi");
    if (rc) return rc;
  }
  return 0;
}

int icl_conv3d_fwd(const float* x, const float* wp, const float* bias, float* y, void* ws, int n, int cin, int cout, int d, int h,
                   int w, int ks, int64_t x_bstride, int64_t y_bstride, void* stream) {
  if (!x || !wp || !y || n < 1 || cin < 1 || cout < 1 || d < 1 || h < 1 || w < 1) return fail(-1, "conv3d_fwd: bad argument");
  const ConvArgs a{x, wp, bias, y, x_bstride, y_bstride, (hipStream_t)stream};
  if (ks == 3) return conv_fwd_launch<3>({n, cin, cout, d, h, w}, a, (float*)ws);
  if (ks == 1) return conv_fwd_launch<1>({n, cin, cout, d, h, w}, a, (float*)ws);
  return fail(-1, "conv3d_fwd: kernel size %d unsupported", ks);
}

int64_t icl_conv3d_fwd_ws_bytes(int n, int cin, int cout, int d, int h, int w, int ks) {
  if (n < 1 || cin < 1 || cout < 1 || d < 1 || h < 1 || w < 1 || (ks != 1 && ks != 3)) return 0;
  const ConvShape s{n, cin, cout, d, h, w};
  const ConvEnv e = conv_env();
  if (ks == 3) {      // the split-product path may hand a call back to the fp32 kernels (alignment of the actual pointers): cover both plans
    const SplitPlan p = plan_conv_split(s, e);
    const int64_t split = p.ok ? p.w_bytes + p.slab_bytes : 0, fp32 = plan_conv_fp32<3>(s, e).slab_bytes;
    return split > fp32 ? split : fp32;
  }
  return plan_conv_fp32<1>(s, e).slab_bytes;
}

int64_t icl_conv3d_wgrad_ws_bytes(int n, int cin, int cout, int ks) {
  // the launcher may group up to three 16-cout blocks per workgroup (fewer pairs -> more tile splits -> more slabs): size for that
  const int pairs = ks == 3 ? ((round_up(cout, 16) + 47) / 48) * ((round_up(cin, 4) + 15) / 16)
                            : (round_up(cout, 16) / 16) * ((round_up(cin, 4) + 15) / 16);
  return (int64_t)n * wgrad_max_split(pairs, n) * (ks == 1 ? kConvWaves : kWgradWaveGroups) * icl_conv3d_packed_elems(cout, cin, ks, 0) * 4;
}

static bool wgrad_reduce_tall(int nslabs, long pe_all) {
  static const int tall_min = [] { const char* e = getenv("ICL_WGRAD_TALL_MIN"); return e ? atoi(e) : 64; }();   // tests lower it
  return nslabs >= tall_min && pe_all <= (1L << 18);   // many slabs of few elements: 16 slab lanes per element instead of 4
}

// the slabs of a weight gradient; n_live < n: samples [n_live, n) of gy are exactly zero (wgrad_live_prefix)
static int wgrad_slabs_run(const float* x, const float* gy, void* ws, int n, int n_live, int cin, int cout, int d, int h, int w, int ks,
                           int64_t x_bstride, int64_t gy_bstride, int32_t* nslabs, void* stream) {
  if (!x || !gy || !ws || !nslabs || n < 1 || cin < 1 || cout < 1 || (ks != 1 && ks != 3)) return fail(-1, "conv3d_wgrad_slabs: bad argument");
  int ns = 0;
  const int rc = ks == 3 ? conv_wgrad_launch<3>(x, gy, (float*)ws, n, n_live, cin, cout, d, h, w, x_bstride, gy_bstride, &ns, (hipStream_t)stream)
                         : conv_wgrad_launch<1>(x, gy, (float*)ws, n, n_live, cin, cout, d, h, w, x_bstride, gy_bstride, &ns, (hipStream_t)stream);
  *nslabs = ns;
  return rc;
}

int icl_conv3d_wgrad_slabs(const float* x, const float* gy, void* ws, int n, int cin, int cout, int d, int h, int w, int ks,
                           int64_t x_bstride, int64_t gy_bstride, int32_t* nslabs, void* stream) {
  return wgrad_slabs_run(x, gy, ws, n, n, cin, cout, d, h, w, ks, x_bstride, gy_bstride, nslabs, stream);
}

int icl_conv3d_wgrad_reduce_multi(const void* const* ws, void* const* gw, const int32_t* cout, const int32_t* cin, const int32_t* ks,
                                  const int32_t* nslabs, int count, void* stream) {
  if (!ws || !gw || !cout || !cin || !ks || !nslabs || count < 1) return fail(-1, "conv3d_wgrad_reduce_multi: bad argument");
  for (int base = 0; base < count; base += icl::kReduceMulti) {
    icl::ReduceMulti m{};
    const int k = count - base < icl::kReduceMulti ? count - base : icl::kReduceMulti;
    long most = 1;
    for (int i = 0; i < k; ++i) {
      const int j = base + i;
      if (!ws[j] || !gw[j] || cout[j] < 1 || cin[j] < 1 || (ks[j] != 1 && ks[j] != 3) || nslabs[j] < 1)
        return fail(-1, "conv3d_wgrad_reduce_multi: bad job %d", j);
      const long pe = icl_conv3d_packed_elems(cout[j], cin[j], ks[j], 0);
      m.gwp[i] = (const float*)ws[j]; m.gw[i] = (float*)gw[j];
      m.cout[i] = cout[j]; m.cin[i] = cin[j]; m.taps[i] = ks[j] * ks[j] * ks[j]; m.nslabs[i] = nslabs[j];
      m.tall[i] = wgrad_reduce_tall(nslabs[j], pe) ? 1 : 0;
      const long blocks = m.tall[i] ? cdivl(pe, 16) : cdivl(pe, 64);
      if (blocks > most) most = blocks;
    }
    ICL_LAUNCH(icl::reduce_unpack_wgrad_multi_kernel, dim3((unsigned)(most < 1024 ? most : 1024), k), dim3(256), 0, (hipStream_t)stream, m);
    const int rc = check_launch("reduce_unpack_wgrad_multi");
    if (rc) return rc;
  }
  return 0;
}

static int wgrad_run(const float* x, const float* gy, float* gw, float* gbias, void* ws, int n, int n_live, int cin, int cout, int d,
                     int h, int w, int ks, int64_t x_bstride, int64_t gy_bstride, void* stream) {
  if (!x || !gy || !gw || !ws || n < 1 || cin < 1 || cout < 1 || (ks != 1 && ks != 3)) return fail(-1, "conv3d_wgrad: bad argument");
  hipStream_t s = (hipStream_t)stream;
  float* gwp = (float*)ws;
  int nslabs = 0;
  int rc = ks == 3 ? conv_wgrad_launch<3>(x, gy, gwp, n, n_live, cin, cout, d, h, w, x_bstride, gy_bstride, &nslabs, s)
                   : conv_wgrad_launch<1>(x, gy, gwp, n, n_live, cin, cout, d, h, w, x_bstride, gy_bstride, &nslabs, s);
  if (rc) return rc;
  const int T = ks * ks * ks;
  const long pe_all = icl_conv3d_packed_elems(cout, cin, ks, 0);
  if (wgrad_reduce_tall(nslabs, pe_all))
    ICL_LAUNCH(icl::reduce_unpack_wgrad_tall_kernel, dim3((unsigned)cdivl(pe_all, 16)), dim3(256), 0, s, (const float*)gwp, gw, cout, cin, T,
               round_up(cin, 4), round_up(cout, 16), nslabs);
  else
    ICL_LAUNCH(icl::reduce_unpack_wgrad_kernel, dim3(grid_for(pe_all, 64)), dim3(256), 0, s, (const float*)gwp, gw, cout, cin, T,
               round_up(cin, 4), round_up(cout, 16), nslabs);
  rc = check_launch("reduce_unpack_wgrad");
  if (rc) return rc;
  if (gbias) {
    // per-chunk partial sums into the slab workspace (free again: the slabs have been reduced on this stream), then their column
    // sums in a fixed order — no float atomics.  The workspace holds >= n * 32 * round_up(cout, 16) floats (ks 1; far more for ks 3).
    const long S = (long)d * h * w;
    long chunks = cdivl(S, 16384);
    if (chunks > 16) chunks = 16;
    const long clen = round_up(cdivl(S, chunks), 4);
    chunks = cdivl(S, clen);
    float* part = (float*)ws;
    dim3 grid((unsigned)chunks, cout, n);
    ICL_LAUNCH(icl::channel_sum_kernel, grid, dim3(256), 0, s, gy, part, S, (long)gy_bstride, clen);
    rc = check_launch("channel_sum");
    if (rc) return rc;
    const void* g[1] = {part};
    void* out[1] = {gbias};
    const int32_t rr[1] = {(int32_t)(n * chunks)}, cc[1] = {cout};
    rc = icl_colsum_multi(g, out, rr, cc, 1, stream);
  }
  return rc;
}

int icl_conv3d_wgrad(const float* x, const float* gy, float* gw, float* gbias, void* ws, int n, int cin, int cout, int d,
                     int h, int w, int ks, int64_t x_bstride, int64_t gy_bstride, void* stream) {
  return wgrad_run(x, gy, gw, gbias, ws, n, n, cin, cout, d, h, w, ks, x_bstride, gy_bstride, stream);
}

int64_t icl_norm_ws_bytes(int n, int c, int64_t s) {
  const int64_t nch = (s + icl::kNormChunk - 1) / icl::kNormChunk;
  return ((int64_t)n * c * nch * 3 + (int64_t)n * c * 2 + 64) * 4;
}

int icl_norm_fwd(const float* x, float* y, float* mean, float* rstd, const float* gamma, const float* beta,
                 float* running_mean, float* running_var, int n, int c, int64_t s, int mode, int use_batch_stats,
                 int act, float eps, float momentum, void* ws, void* stream) {
  return icl_norm_res_fwd(x, nullptr, y, mean, rstd, gamma, beta, running_mean, running_var, n, c, s, mode, use_batch_stats, act,
                          eps, momentum, ws, stream);
}

int icl_norm_res_fwd(const float* x, const float* res, float* y, float* mean, float* rstd, const float* gamma, const float* beta,
                     float* running_mean, float* running_var, int n, int c, int64_t s, int mode, int use_batch_stats,
                     int act, float eps, float momentum, void* ws, void* stream) {
  if (!x || !y || !mean || !rstd || n < 1 || c < 1 || s < 1) return fail(-1, "norm_fwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const int R = n * c;
  const int nch = (int)((s + icl::kNormChunk - 1) / icl::kNormChunk);
  const float* part = nullptr;
  // instance statistics of rows that are one chunk (the 12^3 / 6^3 levels): summarised inside the normalisation launch
  const int inline_stats = (use_batch_stats && mode == 0 && nch == 1 && !running_mean) ? 1 : 0;
  if (use_batch_stats && !inline_stats) {
    if (!ws) return fail(-1, "norm_fwd: workspace required");
    ICL_LAUNCH(icl::rowstats_partial_kernel, dim3(nch, R), dim3(icl::kNormThreads), 0, st, x, (float*)ws, (long)s, nch);
    if (int rc = check_launch("rowstats_partial")) return rc;
    part = (const float*)ws;
  }
  ICL_LAUNCH(icl::norm_act_fwd_kernel, dim3(nch, R), dim3(icl::kNormThreads), 0, st, x, y, mean, rstd, gamma, beta, (long)s, c, mode, act, res,
             part, R, nch, eps, running_mean, running_var, momentum, inline_stats);
  return check_launch("norm_act_fwd");
}

int icl_norm_fwd_given_stats(const float* x, const float* res, float* y, float* mean, float* rstd, const float* gamma, const float* beta,
                             float* running_mean, float* running_var, int n, int c, int64_t s, int mode, int act, float eps,
                             float momentum, const float* part, int nslots, void* stream) {
  if (!x || !y || !mean || !rstd || !part || n < 1 || c < 1 || s < 1 || nslots < 1) return fail(-1, "norm_fwd_given_stats: bad argument");
  const int R = n * c;
  const int nch = (int)((s + icl::kNormChunk - 1) / icl::kNormChunk);
  ICL_LAUNCH(icl::norm_act_fwd_kernel, dim3(nch, R), dim3(icl::kNormThreads), 0, (hipStream_t)stream, x, y, mean, rstd, gamma, beta, (long)s, c,
             mode, act, res, part, R, nslots, eps, running_mean, running_var, momentum, 0);
  return check_launch("norm_act_fwd");
}

int icl_norm_bwd(const float* gy, const float* x, const float* mean, const float* rstd, const float* gamma,
                 const float* beta, float* gx, float* dgamma, float* dbeta, int n, int c, int64_t s, int mode,
                 int use_batch_stats, int act, void* ws, void* stream) {
  return icl_norm_res_bwd(gy, x, nullptr, mean, rstd, gamma, beta, gx, nullptr, dgamma, dbeta, n, c, s, mode, use_batch_stats, act,
                          ws, stream);
}

int icl_norm_res_bwd(const float* gy, const float* x, const float* res, const float* mean, const float* rstd, const float* gamma,
                     const float* beta, float* gx, float* gres, float* dgamma, float* dbeta, int n, int c, int64_t s, int mode,
                     int use_batch_stats, int act, void* ws, void* stream) {
  if (!gy || !x || !mean || !rstd || !gx || !ws || n < 1 || c < 1 || s < 1) return fail(-1, "norm_bwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const int R = n * c;
  const int nch = (int)((s + icl::kNormChunk - 1) / icl::kNormChunk);
  float* part = (float*)ws;
  if (mode == 0 && nch == 1) {
    part = nullptr;      // instance statistics, one chunk per row: the apply launch computes the row's two sums itself
  } else {
    ICL_LAUNCH(icl::norm_act_bwd_partial_kernel, dim3(nch, R), dim3(icl::kNormThreads), 0, st, gy, x, mean, rstd, gamma, beta, part,
               (long)s, c, nch, mode, act, res);
    if (int rc = check_launch("norm_bwd_partial")) return rc;
  }
  const float inv_count = 1.0f / (float)((mode ? (int64_t)n : 1) * s);
  ICL_LAUNCH(icl::norm_act_bwd_apply_kernel, dim3(nch, R), dim3(icl::kNormThreads), 0, st, gy, x, mean, rstd, gamma, beta,
             (const float*)part, gx, (long)s, c, mode, act, inv_count, use_batch_stats, res, gres, R, nch, dgamma, dbeta);
  return check_launch("norm_bwd_apply");
}

int icl_rstd_from_var(const float* var, float* rstd, int c, float eps, void* stream) {
  if (!var || !rstd || c < 1) return fail(-1, "rstd_from_var: bad argument");
  ICL_LAUNCH(icl::rstd_from_var_kernel, dim3((c + 63) / 64), dim3(64), 0, (hipStream_t)stream, var, rstd, c, eps);
  return check_launch("rstd_from_var");
}

namespace {
// two x-neighbouring windows per thread (16-byte loads) where the rows allow it; ICL_MAXPOOL_BWD_X2=0 also restores the scalar forward (A/B)
int maxpool2_fwd_run(const float* x, const float* ss, float* y, uint8_t* idx, int64_t nc, int dout, int hout, int wout, int pool_depth,
                     hipStream_t st, const char* what) {
  const long total = nc * dout * hout * wout;
  const char* e_x2 = getenv("ICL_MAXPOOL_BWD_X2");
  if ((wout & 1) == 0 && aligned16(x) && ((uintptr_t)y & 7) == 0 && (e_x2 ? atoi(e_x2) : 1)) {
    note_resample("maxpool2_fwd_x2_kernel");
    ICL_LAUNCH(icl::maxpool2_fwd_x2_kernel, dim3(grid_for(total / 2, 256)), dim3(256), 0, st, x, y, idx, (long)nc, dout, hout, wout, pool_depth, ss);
  } else {
    note_resample("maxpool2_fwd_kernel");
    ICL_LAUNCH(icl::maxpool2_fwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, st, x, y, idx, (long)nc, dout, hout, wout, pool_depth, ss);
  }
  return check_launch(what);
}
}  // namespace

int icl_maxpool2_fwd(const float* x, float* y, uint8_t* idx, int64_t nc, int dout, int hout, int wout, int pool_depth, void* stream) {
  if (!x || !y || !idx || nc < 1 || dout < 1 || hout < 1 || wout < 1 || (pool_depth != 1 && pool_depth != 2)) return fail(-1, "maxpool2_fwd: bad argument");
  return maxpool2_fwd_run(x, nullptr, y, idx, nc, dout, hout, wout, pool_depth, (hipStream_t)stream, "maxpool2_fwd");
}

// ---- deferred InstanceNorm + ReLU (round 5; kernels/norm.h norm_finalize_stats_kernel): the consumers of a RAW convolution output
// whose normalisation is applied while they load it.  `ss` = [samples x channels][2] (scale, shift) from icl_norm_finalize_stats.
int icl_norm_finalize_stats(const float* part, int n, int c, int nslots, float eps, float* mean, float* rstd, float* ss, void* stream) {
  if (!part || !mean || !rstd || !ss || n < 1 || c < 1 || nslots < 1) return fail(-1, "norm_finalize_stats: bad argument");
  ICL_LAUNCH(icl::norm_finalize_stats_kernel, dim3(n * c), dim3(64), 0, (hipStream_t)stream, part, n * c, c, nslots, eps, mean, rstd, ss);
  return check_launch("norm_finalize_stats");
}

// y = relu(fma(x, scale, shift)): the deferred normalisation written out after all (a consumer that cannot apply it on load)
int icl_norm_apply(const float* x, const float* ss, float* y, int n, int c, int64_t s, void* stream) {
  if (!x || !ss || !y || n < 1 || c < 1 || s < 4 || (s & 3) || !aligned16(x) || !aligned16(y)) return fail(-1, "norm_apply: bad argument (s %% 4 == 0)");
  ICL_LAUNCH(icl::copy_rows_norm_kernel, dim3(grid_for((long)n * c * (s >> 2), 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream, x, y, n, c, (long)s,
             (long)c * s, ss);
  return check_launch("norm_apply");
}

int icl_maxpool2_fwd_norm(const float* x, const float* ss, float* y, uint8_t* idx, int64_t nc, int dout, int hout, int wout, int pool_depth,
                          void* stream) {
  if (!x || !ss || !y || !idx || nc < 1 || dout < 1 || hout < 1 || wout < 1 || (pool_depth != 1 && pool_depth != 2))
    return fail(-1, "maxpool2_fwd_norm: bad argument");
  return maxpool2_fwd_run(x, ss, y, idx, nc, dout, hout, wout, pool_depth, (hipStream_t)stream, "maxpool2_fwd_norm");
}

// out[:, :cs] = skip, out[:, cs:] = trilinear 2x of deep ([n, cd, d/2, h/2, w/2] -> [n, cd, d, h, w], align_corners = False): the concat
// buffer of UnetUp3_CT (/root/reference/code/networks/utils.py:264,276) with either source given raw + (scale, shift) (null: as stored).
int icl_upsample2x_concat_norm(const float* skip, const float* skip_ss, const float* deep, const float* deep_ss, float* out, int n, int cs,
                               int cd, int d, int h, int w, void* stream) {
  if (!skip || !deep || !out || n < 1 || cs < 1 || cd < 1 || d < 2 || h < 2 || w < 4 || (d & 1) || (h & 1) || (w & 3))
    return fail(-1, "upsample2x_concat_norm: bad argument (even depth / height, width a multiple of 4)");
  if (!aligned16(skip) || !aligned16(deep) || !aligned16(out)) return fail(-1, "upsample2x_concat_norm: 16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  const long s = (long)d * h * w, obs = (long)(cs + cd) * s;
  const long total = (long)n * cd * s;
  const int di = d / 2, hi = h / 2, wi = w / 2;
  note_resample("%s|%s", skip_ss ? "copy_rows_norm_kernel" : "copy_rows_kernel", wi % 4 == 0 ? "upsample2x_fwd_x4_kernel" : "upsample2x_fwd_kernel");
  if (skip_ss) {
    ICL_LAUNCH(icl::copy_rows_norm_kernel, dim3(grid_for((long)n * cs * (s >> 2), 256, 1 << 16)), dim3(256), 0, st, skip, out, n, cs, s, obs, skip_ss);
  } else {
    ICL_LAUNCH(icl::copy_rows_kernel, dim3(grid_for((long)n * cs * s, 256)), dim3(256), 0, st, skip, out, (long)n, (long)cs * s, (long)cs * s, obs);
  }
  if (int rc = check_launch("upsample2x_concat_norm: skip")) return rc;
  if (wi % 4 == 0)
    ICL_LAUNCH(icl::upsample2x_fwd_x4_kernel, dim3(grid_for(total / 32, 256, 1 << 16)), dim3(256), 0, st, deep, out + (long)cs * s, n, cd, di, hi, wi, obs,
               deep_ss);
  else
    ICL_LAUNCH(icl::upsample2x_fwd_kernel, dim3(grid_for(total / 16, 256, 1 << 16)), dim3(256), 0, st, deep, out + (long)cs * s, n, cd, di, hi, wi, obs,
               deep_ss);
  return check_launch("upsample2x_concat_norm: deep");
}

int icl_maxpool2_bwd(const float* gy, const uint8_t* idx, float* gx, int64_t nc, int dout, int hout, int wout, int pool_depth, void* stream) {
  if (!gy || !gx || !idx || nc < 1 || dout < 1 || hout < 1 || wout < 1 || (pool_depth != 1 && pool_depth != 2)) return fail(-1, "maxpool2_bwd: bad argument");
  const long total = nc * dout * hout * wout;
  note_resample("maxpool2_bwd_kernel");
  ICL_LAUNCH(icl::maxpool2_bwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, gy, idx, gx, (long)nc, dout, hout, wout,
             pool_depth);
  return check_launch("maxpool2_bwd");
}

int icl_maxpool2_bwd_add(const float* gy, const uint8_t* idx, const float* add, float* gx, int n, int c, int dout, int hout, int wout,
                         int pool_depth, int64_t add_bstride, void* stream) {
  return icl_maxpool2_bwd_add_live(gy, idx, add, gx, n, n, c, dout, hout, wout, pool_depth, add_bstride, stream);
}

int icl_maxpool2_bwd_add_live(const float* gy, const uint8_t* idx, const float* add, float* gx, int n, int skip_live, int c, int dout, int hout,
                              int wout, int pool_depth, int64_t add_bstride, void* stream) {
  if (!gy || !gx || !idx || !add || n < 1 || c < 1 || dout < 1 || hout < 1 || wout < 1 || (pool_depth != 1 && pool_depth != 2) || (add_bstride & 1) ||
      ((uintptr_t)add & 7) || skip_live < 1 || skip_live > n)
    return fail(-1, "maxpool2_bwd_add: bad argument");
  const long ncskip = (long)skip_live * c;
  const long total = (long)n * c * dout * hout * wout;
  // two x-neighbouring outputs per thread (16-byte accesses) where the rows allow it; ICL_MAXPOOL_BWD_X2=0: the 8-byte form (A/B)
  const char* e_x2 = getenv("ICL_MAXPOOL_BWD_X2");
  if ((wout & 1) == 0 && aligned16(add) && aligned16(gx) && ((uintptr_t)gy & 7) == 0 && (add_bstride & 3) == 0 && (e_x2 ? atoi(e_x2) : 1)) {
    note_resample("maxpool2_bwd_add_x2_kernel");
    ICL_LAUNCH(icl::maxpool2_bwd_add_x2_kernel, dim3(grid_for(total / 2, 256)), dim3(256), 0, (hipStream_t)stream, gy, idx, add, gx, (long)n * c, c,
               dout, hout, wout, pool_depth, (long)add_bstride, ncskip);
    return check_launch("maxpool2_bwd_add_x2");
  }
  note_resample("maxpool2_bwd_add_kernel");
  ICL_LAUNCH(icl::maxpool2_bwd_add_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, gy, idx, add, gx, (long)n * c, c, dout,
             hout, wout, pool_depth, (long)add_bstride, ncskip);
  return check_launch("maxpool2_bwd_add");
}

namespace {
inline float resize_scale(int in, int out, int align) {
  if (align) return out > 1 ? (float)(in - 1) / (float)(out - 1) : 0.f;
  return (float)in / (float)out;
}
}  // namespace

int icl_trilinear_fwd(const float* x, float* y, int n, int c, int di, int hi, int wi, int dout, int hout, int wout,
                      int64_t y_bstride, int align_corners, void* stream) {
  if (!x || !y || n < 1 || c < 1 || di < 1 || hi < 1 || wi < 1 || dout < 1 || hout < 1 || wout < 1) return fail(-1, "trilinear_fwd: bad argument");
  const long total = (long)n * c * dout * hout * wout;
  const float rz = resize_scale(di, dout, align_corners), ry = resize_scale(hi, hout, align_corners), rx = resize_scale(wi, wout, align_corners);
  if (!align_corners && dout == 2 * di && hout == 2 * hi && wout == 2 * wi && wi % 2 == 0 && y_bstride % 4 == 0 && aligned16(y) &&
      total / 16 < (1L << 31)) {   // the decoder's exact 2x upsampling: 2 x 2 x 4 outputs per thread, 2 x 2 x 8 where the rows allow 16-byte loads
    constexpr int x4 = 1;
    note_resample(x4 && wi % 4 == 0 && aligned16(x) ? "upsample2x_fwd_x4_kernel" : "upsample2x_fwd_kernel");
    if (x4 && wi % 4 == 0 && aligned16(x))
      ICL_LAUNCH(icl::upsample2x_fwd_x4_kernel, dim3(grid_for(total / 32, 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream, x, y, n, c, di, hi,
                 wi, (long)y_bstride, (const float*)nullptr);
    else
      ICL_LAUNCH(icl::upsample2x_fwd_kernel, dim3(grid_for(total / 16, 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream, x, y, n, c, di, hi, wi,
                 (long)y_bstride, (const float*)nullptr);
  } else if (wout % 4 == 0 && y_bstride % 4 == 0 && aligned16(y) && total / 4 < (1L << 31)) {
    note_resample("trilinear_fwd_quad_kernel");
    ICL_LAUNCH(icl::trilinear_fwd_quad_kernel, dim3(grid_for(total / 4, 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream, x, y, n, c, di, hi,
               wi, dout, hout, wout, rz, ry, rx, (long)y_bstride, align_corners);
  } else {
    note_resample("trilinear_fwd_kernel");
    ICL_LAUNCH(icl::trilinear_fwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, x, y, n, c, di, hi, wi, dout, hout,
               wout, rz, ry, rx, (long)y_bstride, align_corners);
  }
  return check_launch("trilinear_fwd");
}

int64_t icl_trilinear_bwd_ws_bytes(int n, int c, int di, int hi, int wi, int dout, int hout, int wout) {
  (void)di;
  return ((int64_t)n * c * dout * hout * wi + (int64_t)n * c * dout * hi * wi) * 4;
}

int icl_trilinear_bwd(const float* gy, float* gx, void* ws, int n, int c, int di, int hi, int wi, int dout, int hout, int wout,
                      int64_t gy_bstride, int align_corners, void* stream) {
  if (!gy || !gx || !ws || n < 1 || c < 1 || di < 1 || hi < 1 || wi < 1 || dout < 1 || hout < 1 || wout < 1) return fail(-1, "trilinear_bwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const int al = align_corners;
  const float rz = resize_scale(di, dout, al), ry = resize_scale(hi, hout, al), rx = resize_scale(wi, wout, al);
  float* t1 = (float*)ws;                                  // [n][c*dout*hout][wi]
  float* t2 = t1 + (size_t)n * c * dout * hout * wi;       // [n][c*dout][hi][wi]
  int rc;
  if (!al && dout == 2 * di && hout == 2 * hi && wout == 2 * wi && wi % 4 == 0 && gy_bstride % 4 == 0 && aligned16(gy) && aligned16(gx) &&
      (long)n * c * di * hi * wi / 4 < (1L << 31)) {   // exact 2x: one pass, four inputs per thread, no workspace traffic
    note_resample("upsample2x_bwd_kernel");
    ICL_LAUNCH(icl::upsample2x_bwd_kernel, dim3(grid_for((long)n * c * ((di + icl::kUpSeg - 1) / icl::kUpSeg) * hi * wi / 4, 256, 1 << 16)),
               dim3(256), 0, st, gy, gx, n, c, di, hi,
               wi, (long)gy_bstride);
    return check_launch("upsample2x_bwd");
  }
  // one axis per launch; the vectorised kernels need 16-byte rows and a quad count that fits 32 bits
  const char* used[3] = {"", "", ""};   // the kernel of each axis pass, for the route record
  int pass = 0;
  auto axis = [&](const float* src, float* dst, long rows, int li, int lo, long inner, float rs, long sbs, const char* what) -> int {
    const long total = (long)n * rows * li * inner;
    const bool small = total / 4 < (1L << 31) && rows < (1L << 31);
    if (small && inner % 4 == 0 && sbs % 4 == 0 && aligned16(src) && aligned16(dst)) {
      used[pass++] = "resize_bwd_axis_t4_kernel";
      ICL_LAUNCH(icl::resize_bwd_axis_t4_kernel, dim3(grid_for(total / 4, 256, 1 << 16)), dim3(256), 0, st, src, dst, n, (unsigned)rows, li, lo,
                 (unsigned)(inner / 4), rs, sbs, al);
    } else if (inner == 1 && lo >= 4 * li && lo % 4 == 0 && lo <= 1024 && sbs % 4 == 0 && aligned16(src) && rows * li >= 4096) {
      // big x pass of a >= 4x upscale: rows of dY staged in LDS with coalesced loads
      const long nrows = (long)n * rows;
      used[pass++] = "resize_bwd_axis_x_lds_kernel";
      ICL_LAUNCH(icl::resize_bwd_axis_x_lds_kernel, dim3((unsigned)cdivl(nrows, icl::kRbxRows)), dim3(256),
                 (size_t)icl::kRbxRows * (lo + 4) * 4, st, src, dst, n, rows, li, lo, rs, sbs, al);
    } else if (small && inner == 1 && li % 4 == 0 && aligned16(dst)) {
      used[pass++] = "resize_bwd_axis_i4_kernel";
      ICL_LAUNCH(icl::resize_bwd_axis_i4_kernel, dim3(grid_for(total / 4, 256, 1 << 16)), dim3(256), 0, st, src, dst, n, (unsigned)rows, li, lo,
                 rs, sbs, al);
    } else {
      used[pass++] = "resize_bwd_axis_kernel";
      ICL_LAUNCH(icl::resize_bwd_axis_kernel, dim3(grid_for(total, 256)), dim3(256), 0, st, src, dst, n, rows, li, lo, inner, rs, sbs, al);
    }
    note_resample("x:%s|y:%s|z:%s", used[0], used[1], used[2]);
    return check_launch(what);
  };
  if ((rc = axis(gy, t1, (long)c * dout * hout, wi, wout, 1L, rx, (long)gy_bstride, "resize_bwd_x"))) return rc;
  if ((rc = axis(t1, t2, (long)c * dout, hi, hout, (long)wi, ry, (long)c * dout * hout * wi, "resize_bwd_y"))) return rc;
  if ((rc = axis(t2, gx, (long)c, di, dout, (long)hi * wi, rz, (long)c * dout * hi * wi, "resize_bwd_z"))) return rc;
  return 0;
}

int icl_copy_rows(const float* src, float* dst, int64_t rows, int64_t row_elems, int64_t src_stride, int64_t dst_stride,
                  void* stream) {
  if (!src || !dst || rows < 1 || row_elems < 1) return fail(-1, "copy_rows: bad argument");
  ICL_LAUNCH(icl::copy_rows_kernel, dim3(grid_for(rows * row_elems, 256)), dim3(256), 0, (hipStream_t)stream, src, dst, (long)rows,
             (long)row_elems, (long)src_stride, (long)dst_stride);
  return check_launch("copy_rows");
}

int icl_concat2(const float* a, int64_t na, const float* b, int64_t nb, float* out, void* stream) {
  if (!out || na < 0 || nb < 0 || na + nb < 4 || (na & 3) || (nb & 3) || (!a && !b)) return fail(-1, "concat2: bad argument (float counts are multiples of 4)");
  if ((a && !aligned16(a)) || (b && !aligned16(b)) || !aligned16(out)) return fail(-1, "concat2: 16-byte alignment");
  ICL_LAUNCH(icl::concat2_kernel, dim3(grid_for((na + nb) >> 2, 256)), dim3(256), 0, (hipStream_t)stream, a, (long)na, b, (long)nb, out);
  return check_launch("concat2");
}

int icl_depth_to_space2(const float* yt, float* out, int n, int d, int h, int w, int cout, int64_t out_bstride, void* stream) {
  if (!yt || !out || n < 1 || d < 1 || h < 1 || w < 1 || cout < 1) return fail(-1, "depth_to_space2: bad argument");
  const size_t lds = (size_t)w * (cout * 8 + 2) * 4;
  if (lds > (size_t)kMaxDynLdsBig) return fail(-1, "depth_to_space2: token row does not fit LDS (w * cout too large)");
  if (lds > (size_t)kMaxDynLds) ICL_SET_MAX_DYN_LDS(icl::depth_to_space2_kernel, kMaxDynLdsBig);
  note_resample("depth_to_space2_kernel%s", lds > (size_t)kMaxDynLds ? "+big_lds" : "+lds");
  ICL_LAUNCH(icl::depth_to_space2_kernel, dim3(h, d, n), dim3(256), lds, (hipStream_t)stream, yt, out, d, h, w, cout, (long)out_bstride);
  return check_launch("depth_to_space2");
}

int icl_space_to_depth2(const float* g, float* gt, int n, int d, int h, int w, int cout, int64_t g_bstride, void* stream) {
  if (!g || !gt || n < 1 || d < 1 || h < 1 || w < 1 || cout < 1) return fail(-1, "space_to_depth2: bad argument");
  const size_t lds = (size_t)w * (cout * 8 + 2) * 4;
  if (lds > (size_t)kMaxDynLdsBig) return fail(-1, "space_to_depth2: token row does not fit LDS (w * cout too large)");
  if (lds > (size_t)kMaxDynLds) ICL_SET_MAX_DYN_LDS(icl::space_to_depth2_kernel, kMaxDynLdsBig);
  note_resample("space_to_depth2_kernel%s", lds > (size_t)kMaxDynLds ? "+big_lds" : "+lds");
  ICL_LAUNCH(icl::space_to_depth2_kernel, dim3(h, d, n), dim3(256), lds, (hipStream_t)stream, g, gt, d, h, w, cout, (long)g_bstride);
  return check_launch("space_to_depth2");
}

int icl_dwconv3_fwd(const float* x, const float* w, float* y, int n, int c, int d, int h, int wd, int flip, void* stream) {
  if (!x || !w || !y || n < 1 || c < 1 || d < 1 || h < 1 || wd < 1) return fail(-1, "dwconv3_fwd: bad argument");
  const long total = (long)n * c * d * h * wd;
  ICL_LAUNCH(icl::dwconv3_fwd_kernel, dim3(grid_for(total, 256)), dim3(256), 0, (hipStream_t)stream, x, w, y, (long)n * c, c, d, h, wd, flip);
  return check_launch("dwconv3_fwd");
}

static long dwconv3_wgrad_chunks(long total) {
  long chunks = cdivl(total, 1024);   // >= 4 voxels per thread; the aligner maps are tiny (<= 4 x 24^3): parallelism over reuse
  return chunks > 512 ? 512 : chunks;   // (64 until round 6: SwinUNETR's 48^3 maps, 442 k voxels per channel, ran 27 voxels x 27 taps per thread)
}

int64_t icl_dwconv3_wgrad_ws_bytes(int n, int c, int d, int h, int wd) {
  return dwconv3_wgrad_chunks((long)n * d * h * wd) * c * 27 * 4;
}

int icl_dwconv3_wgrad(const float* x, const float* gy, float* gw, void* ws, int n, int c, int d, int h, int wd, void* stream) {
  if (!x || !gy || !gw || !ws || n < 1 || c < 1 || d < 1 || h < 1 || wd < 1) return fail(-1, "dwconv3_wgrad: bad argument");
  hipStream_t s = (hipStream_t)stream;
  const long total = (long)n * d * h * wd;
  const long chunks = dwconv3_wgrad_chunks(total);
  const long chunk = cdivl(total, chunks);
  ICL_LAUNCH(icl::dwconv3_wgrad_kernel, dim3((unsigned)chunks, c), dim3(256), 0, s, x, gy, (float*)ws, n, c, d, h, wd, chunk);
  if (int rc = check_launch("dwconv3_wgrad")) return rc;
  ICL_LAUNCH(icl::dwconv3_wgrad_reduce_kernel, dim3((unsigned)cdivl((long)c * 27, 16)), dim3(256), 0, s, (const float*)ws, gw, c * 27, (int)chunks);
  return check_launch("dwconv3_wgrad_reduce");
}

namespace {
icl::DropSpec drop_spec(int mode, uint32_t seed, float p, const uint32_t* seed_dev) {
  icl::DropSpec d{};
  d.mode = mode;
  d.seed = (unsigned)seed;
  d.thresh = (unsigned)((double)p * 4294967296.0);      // as icl_drop_path_add
  d.scale = 1.0f / (1.0f - p);
  d.seed_dev = (const unsigned*)seed_dev;
  return d;
}

// n_plan: the batch size the kernel is chosen for (a live batch runs the kernel of its full batch: the same bits per sample); 0: n
int conv1x1_small_run(const float* x, const float* w, const float* bias, float* y, int n, int cin, int cout, int64_t s, int w_ostride,
                      int w_istride, const icl::DropSpec& dr, hipStream_t st, int n_plan = 0) {
  if ((long)(n_plan > n ? n_plan : n) * s >= 65536) {   // big volume: every input value loaded once per group of <= 16 outputs
    const long quads = (long)n * (s >> 2);
    const int ob = cout <= 1 ? 1 : cout <= 2 ? 2 : cout <= 4 ? 4 : cout <= 8 ? 8 : 16;
    const dim3 grid(grid_for(quads, 256, 1 << 16), (cout + ob - 1) / ob);
    switch (ob) {
      case 1: ICL_LAUNCH(icl::conv1x1_stream_kernel<1>, grid, dim3(256), 0, st, x, w, bias, y, n, cin, cout, (long)s, w_ostride, w_istride, dr); break;
      case 2: ICL_LAUNCH(icl::conv1x1_stream_kernel<2>, grid, dim3(256), 0, st, x, w, bias, y, n, cin, cout, (long)s, w_ostride, w_istride, dr); break;
      case 4: ICL_LAUNCH(icl::conv1x1_stream_kernel<4>, grid, dim3(256), 0, st, x, w, bias, y, n, cin, cout, (long)s, w_ostride, w_istride, dr); break;
      case 8: ICL_LAUNCH(icl::conv1x1_stream_kernel<8>, grid, dim3(256), 0, st, x, w, bias, y, n, cin, cout, (long)s, w_ostride, w_istride, dr); break;
      default: ICL_LAUNCH(icl::conv1x1_stream_kernel<16>, grid, dim3(256), 0, st, x, w, bias, y, n, cin, cout, (long)s, w_ostride, w_istride, dr); break;
    }
    return check_launch("conv1x1_stream");
  }
  if (dr.mode) return 1;      // the small-volume kernel has no mask: the caller runs dropout and convolution apart
  const long total = (long)n * cout * (s >> 2);
  ICL_LAUNCH(icl::conv1x1_small_kernel, dim3(grid_for(total, 256)), dim3(256), 0, st, x, w, bias, y, n, cin, cout, (long)s,
             w_ostride, w_istride);
  return check_launch("conv1x1_small");
}
}  // namespace

int icl_conv1x1_small(const float* x, const float* w, const float* bias, float* y, int n, int cin, int cout, int64_t s, int w_ostride,
                      int w_istride, void* stream) {
  if (!x || !w || !y || n < 1 || cin < 1 || cout < 1 || s < 4 || (s & 3)) return fail(-1, "conv1x1_small: bad argument (s %% 4 == 0)");
  return conv1x1_small_run(x, w, bias, y, n, cin, cout, s, w_ostride, w_istride, icl::DropSpec{}, (hipStream_t)stream);
}

// The same with nn.Dropout(p) folded in (the counter-based mask of icl_dropout, same seed protocol): mask_mode 1 = the INPUT is the dropped
// tensor (y = conv(dropout(x)): `final(dropout2(up1))`), 2 = the OUTPUT is (the input gradient of that pair: gx = dropout'(conv^T gy)).
// Returns 1 without launching for volumes the big-volume kernel does not take (n * s < 65536).
int icl_conv1x1_dropout(const float* x, const float* w, const float* bias, float* y, int n, int cin, int cout, int64_t s, int w_ostride,
                        int w_istride, int mask_mode, uint32_t seed, float p, const uint32_t* seed_dev, void* stream) {
  if (!x || !w || !y || n < 1 || cin < 1 || cout < 1 || s < 4 || (s & 3) || (mask_mode != 1 && mask_mode != 2) || !(p >= 0.f && p < 1.f))
    return fail(-1, "conv1x1_dropout: bad argument");
  return conv1x1_small_run(x, w, bias, y, n, cin, cout, s, w_ostride, w_istride, drop_spec(mask_mode, seed, p, seed_dev), (hipStream_t)stream);
}

// y = conv1x1(dropout(relu(fma(x, scale, shift)), p)): `final(dropout2(up1))` with up1 given as the raw output of its last convolution
// (unet_3D_icl.py:67-68,116-117; p = 0: no mask — evaluation).  Forward only; the input gradient is icl_conv1x1_dropout(mask_mode 2).
int icl_conv1x1_dropout_norm(const float* x, const float* ss, const float* w, const float* bias, float* y, int n, int cin, int cout, int64_t s,
                             int w_ostride, int w_istride, uint32_t seed, float p, const uint32_t* seed_dev, void* stream) {
  if (!x || !ss || !w || !y || n < 1 || cin < 1 || cout < 1 || s < 4 || (s & 3) || !(p >= 0.f && p < 1.f) || (long)n * s < 65536)
    return fail(-1, "conv1x1_dropout_norm: bad argument (big volumes only: n * s >= 65536)");
  icl::DropSpec dr = p > 0.f ? drop_spec(1, seed, p, seed_dev) : icl::DropSpec{};
  dr.ss = ss;
  return conv1x1_small_run(x, w, bias, y, n, cin, cout, s, w_ostride, w_istride, dr, (hipStream_t)stream);
}

int icl_scalar_combine(const void* const* in, const float* w, int n_in, int n_out, float* out, void* stream) {
  if (!in || !w || !out || n_in < 1 || n_out < 1 || n_in > icl::kScalarCombine || n_out > icl::kScalarCombine)
    return fail(-1, "scalar_combine: bad argument (<= %d scalars in and out)", icl::kScalarCombine);
  icl::ScalarCombine s{};
  s.n_in = n_in; s.n_out = n_out;
  for (int i = 0; i < n_in; ++i) {
    if (!in[i]) return fail(-1, "scalar_combine: null input %d", i);
    s.in[i] = (const float*)in[i];
  }
  for (int j = 0; j < n_out; ++j)
    for (int i = 0; i < n_in; ++i) s.w[j][i] = w[j * n_in + i];      // host array, row-major [n_out][n_in]
  ICL_LAUNCH(icl::scalar_combine_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, s, out);
  return check_launch("scalar_combine");
}

int icl_colsum_multi(const void* const* g, void* const* out, const int32_t* rows, const int32_t* cols, int count, void* stream) {
  if (!g || !out || !rows || !cols || count < 1) return fail(-1, "colsum_multi: bad argument");
  for (int base = 0; base < count; base += icl::kColsumMulti) {
    icl::ColsumMulti m{};
    const int k = count - base < icl::kColsumMulti ? count - base : icl::kColsumMulti;
    int cmax = 1;
    for (int i = 0; i < k; ++i) {
      const int j = base + i;
      if (!g[j] || !out[j] || rows[j] < 1 || cols[j] < 1) return fail(-1, "colsum_multi: bad tensor %d", j);
      m.g[i] = (const float*)g[j]; m.out[i] = (float*)out[j]; m.rows[i] = rows[j]; m.cols[i] = cols[j];
      if (cols[j] > cmax) cmax = cols[j];
    }
    ICL_LAUNCH(icl::colsum_multi_kernel, dim3(grid_for(cmax, 16, 128), k), dim3(256), 0, (hipStream_t)stream, m);
    const int rc = check_launch("colsum_multi");
    if (rc) return rc;
  }
  return 0;
}

int icl_gather_rows(const float* src, const int32_t* idx, float* out, int64_t b, int64_t s, int64_t m, int c, void* stream) {
  if (!src || !idx || !out || b < 1 || s < 1 || m < 1 || c < 4 || (c & 3)) return fail(-1, "gather_rows: bad argument (c %% 4 == 0)");
  ICL_LAUNCH(icl::gather_rows_kernel, dim3(grid_for(b * m * (c / 4), 256)), dim3(256), 0, (hipStream_t)stream, src, (const int*)idx, out,
             (long)b, (long)s, (long)m, c / 4);
  return check_launch("gather_rows");
}

int icl_gather_rows_sum2(const float* src, const int32_t* idx2, float* out, int64_t b, int64_t s, int64_t m, int c, void* stream) {
  if (!src || !idx2 || !out || b < 1 || s < 1 || m < 1 || c < 4 || (c & 3)) return fail(-1, "gather_rows_sum2: bad argument (c %% 4 == 0)");
  ICL_LAUNCH(icl::gather_rows_sum2_kernel, dim3(grid_for(b * m * (c / 4), 256)), dim3(256), 0, (hipStream_t)stream, src, (const int*)idx2, out,
             (long)b, (long)s, (long)m, c / 4);
  return check_launch("gather_rows_sum2");
}

int icl_im2col3(const float* x, float* cols, int n, int c, int d, int h, int w, void* stream) {
  if (!x || !cols || n < 1 || c < 1 || d < 1 || h < 1 || w < 1) return fail(-1, "im2col3: bad argument");
  ICL_LAUNCH(icl::im2col3_kernel, dim3(grid_for((long)n * c * 27 * d * h * w, 256)), dim3(256), 0, (hipStream_t)stream, x, cols, n, c, d, h, w);
  return check_launch("im2col3");
}

int icl_im2col3_planes(const float* x, float* planes, int n, int c, int d, int h, int w, void* stream) {
  if (!x || !planes || n < 1 || c < 1 || d < 1 || h < 1 || w < 4 || (w & 3)) return fail(-1, "im2col3_planes: bad argument (w %% 4 == 0)");
  ICL_LAUNCH(icl::im2col3_planes_kernel, dim3(grid_for((long)n * c * 27 * d * h * (w / 4), 256, 1 << 16)), dim3(256), 0, (hipStream_t)stream, x,
             planes, n, c, d, h, w);
  return check_launch("im2col3_planes");
}

int icl_col2im3(const float* g, float* dx, int n, int c, int d, int h, int w, void* stream) {
  if (!g || !dx || n < 1 || c < 1 || d < 1 || h < 1 || w < 1) return fail(-1, "col2im3: bad argument");
  ICL_LAUNCH(icl::col2im3_kernel, dim3(grid_for((long)n * c * d * h * w, 256)), dim3(256), 0, (hipStream_t)stream, g, dx, n, c, d, h, w);
  return check_launch("col2im3");
}

int icl_drop_path_add(const float* x, const float* res, float* y, int64_t n, int64_t group, uint32_t seed, float p,
                      const uint32_t* seed_dev, void* stream) {
  if (!x || !y || n < 1 || group < 1 || !(p >= 0.f && p < 1.f)) return fail(-1, "dropout: bad argument");
  const unsigned thresh = (unsigned)((double)p * 4294967296.0);
  ICL_LAUNCH(icl::dropout_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, x, res, y, (long)n, (unsigned)seed, thresh,
             1.0f / (1.0f - p), (const unsigned*)seed_dev, (long)group);
  return check_launch("dropout");
}

int icl_drop_path(const float* x, float* y, int64_t n, int64_t group, uint32_t seed, float p, const uint32_t* seed_dev, void* stream) {
  return icl_drop_path_add(x, nullptr, y, n, group, seed, p, seed_dev, stream);
}

int icl_dropout(const float* x, float* y, int64_t n, uint32_t seed, float p, const uint32_t* seed_dev, void* stream) {
  return icl_drop_path(x, y, n, 1, seed, p, seed_dev, stream);
}

// Class groups of the loss kernels: 0 = registers, 4 classes; 1 = registers, 16 classes; 2 = the generic-class path (17 .. 256 classes, or any
// count with the test-only override ICL_LOSS_GENERIC=1, read per call: the tests switch it)
static bool loss_force_generic() {
  const char* e = getenv("ICL_LOSS_GENERIC");
  return e && atoi(e) == 1;
}
static int loss_class_group(int nc) { return nc <= 4 ? 0 : (nc <= 16 ? 1 : 2); }

int icl_loss_fwd(const float* a, const float* b, const int64_t* labels, const float* weight, float* stats, float* out,
                 int batch, int nc, int64_t s, int mode, int a_is_prob, void* stream) {
  if (nc < 1 || nc > icl::kLossMaxNc) return fail(-1, "loss_fwd: %d classes (1 .. %d)", nc, icl::kLossMaxNc);
  if (!a || !stats || !out || batch < 1 || s < 1 || mode < 0 || mode > 3) return fail(-1, "loss_fwd: bad argument");
  if ((mode <= 1) != (labels != nullptr) || (mode >= 2) != (b != nullptr)) return fail(-1, "loss_fwd: target does not match mode");
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)batch * s;
  const int nblk = grid_for(total, 256, ICL_LOSS_MAX_BLOCKS);
  float* part = stats + (3 * nc + 1);   // per-block partial sums behind the reduced statistics
  const dim3 grid(nblk), block(256);
  const long long* lab = (const long long*)labels;
  if (nc > 16 || loss_force_generic()) {
    ICL_LAUNCH(icl::loss_stats_generic_kernel, grid, block, 0, st, a, b, lab, part, batch, nc, (long)s, a_is_prob);
  } else if (nc <= 4) {
    ICL_LAUNCH((icl::loss_stats_kernel<4>), grid, block, 0, st, a, b, lab, part, batch, nc, (long)s, a_is_prob);
  } else {
    ICL_LAUNCH((icl::loss_stats_kernel<16>), grid, block, 0, st, a, b, lab, part, batch, nc, (long)s, a_is_prob);
  }
  int rc = check_launch("loss_stats");
  if (rc) return rc;
  ICL_LAUNCH(icl::loss_finalize_kernel, dim3(1), dim3(256), 0, st, (const float*)part, nblk, stats, weight, out, nc, 1.0f / (float)total,
             1.0f / ((float)total * (float)nc), mode);
  return check_launch("loss_finalize");
}

static int loss_multi_fill(const IclLossJob* jobs, int count, bool bwd, icl::LossMulti& m, int& most, int& group) {
  if (!jobs || count < 1 || count > icl::kLossMulti) return fail(-1, "loss_multi: 1 .. %d jobs", icl::kLossMulti);
  most = 1;
  group = loss_class_group(jobs[0].nc);
  for (int j = 0; j < count; ++j) {
    const IclLossJob& q = jobs[j];
    if (q.nc < 1 || q.nc > icl::kLossMaxNc) return fail(-1, "loss_multi: job %d has %d classes (1 .. %d)", j, q.nc, icl::kLossMaxNc);
    if (!q.a || !q.stats || q.batch < 1 || q.s < 1 || q.mode < 0 || q.mode > 3 || loss_class_group(q.nc) != group)
      return fail(-1, "loss_multi: bad job %d (all jobs of a call need nc <= 4, or all 5 .. 16, or all 17 .. %d)", j, icl::kLossMaxNc);
    if ((q.mode <= 1) != (q.labels != nullptr) || (q.mode >= 2) != (q.b != nullptr)) return fail(-1, "loss_multi: target of job %d does not match its mode", j);
    if (bwd ? !q.ga : !q.out) return fail(-1, "loss_multi: job %d has no output", j);
    const long total = (long)q.batch * q.s;
    m.a[j] = q.a; m.b[j] = q.b; m.lab[j] = (const long long*)q.labels; m.weight[j] = q.weight; m.stats[j] = q.stats; m.out[j] = q.out;
    m.g0[j] = q.gout0; m.g1[j] = q.gout1; m.ga[j] = q.ga;
    m.S[j] = (long)q.s; m.B[j] = q.batch; m.nc[j] = q.nc; m.mode[j] = q.mode; m.aip[j] = q.a_is_prob;
    m.nblk[j] = bwd ? grid_for(total, 256, 4096) : grid_for(total, 256, ICL_LOSS_MAX_BLOCKS);      // as icl_loss_bwd / icl_loss_fwd
    if (m.nblk[j] > most) most = m.nblk[j];
  }
  if (loss_force_generic()) group = 2;
  return 0;
}

int icl_loss_fwd_multi(const IclLossJob* jobs, int count, void* stream) {
  icl::LossMulti m{};
  int most = 1, group = 0;
  int rc = loss_multi_fill(jobs, count, false, m, most, group);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (group == 2) {
    ICL_LAUNCH(icl::loss_stats_generic_multi_kernel, dim3(most, count), dim3(256), 0, st, m);
  } else if (group == 0) {
    ICL_LAUNCH((icl::loss_stats_multi_kernel<4>), dim3(most, count), dim3(256), 0, st, m);
  } else {
    ICL_LAUNCH((icl::loss_stats_multi_kernel<16>), dim3(most, count), dim3(256), 0, st, m);
  }
  rc = check_launch("loss_stats_multi");
  if (rc) return rc;
  ICL_LAUNCH(icl::loss_finalize_multi_kernel, dim3(count), dim3(256), 0, st, m);
  return check_launch("loss_finalize_multi");
}

int icl_loss_bwd_multi(const IclLossJob* jobs, int count, void* stream) {
  icl::LossMulti m{};
  int most = 1, group = 0;
  int rc = loss_multi_fill(jobs, count, true, m, most, group);
  if (rc) return rc;
  if (group == 2) {
    ICL_LAUNCH(icl::loss_grad_generic_multi_kernel, dim3(most, count), dim3(256), 0, (hipStream_t)stream, m);
  } else if (group == 0) {
    ICL_LAUNCH((icl::loss_grad_multi_kernel<4>), dim3(most, count), dim3(256), 0, (hipStream_t)stream, m);
  } else {
    ICL_LAUNCH((icl::loss_grad_multi_kernel<16>), dim3(most, count), dim3(256), 0, (hipStream_t)stream, m);
  }
  return check_launch("loss_grad_multi");
}

int icl_loss_bwd(const float* a, const float* b, const int64_t* labels, const float* weight, const float* stats,
                 const float* gout0, const float* gout1, float* ga, int batch, int nc, int64_t s, int mode, int a_is_prob,
                 void* stream) {
  if (nc < 1 || nc > icl::kLossMaxNc) return fail(-1, "loss_bwd: %d classes (1 .. %d)", nc, icl::kLossMaxNc);
  if (!a || !stats || !ga || batch < 1 || s < 1) return fail(-1, "loss_bwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)batch * s;
  const float inv_vox = 1.0f / (float)total, inv_elems = 1.0f / ((float)total * (float)nc);
  const dim3 grid(grid_for(total, 256, 4096)), block(256);
  const long long* lab = (const long long*)labels;
  if (nc > 16 || loss_force_generic()) {
    ICL_LAUNCH(icl::loss_grad_generic_kernel, grid, block, 0, st, a, b, lab, stats, weight, gout0, gout1, ga, batch, nc, (long)s, mode, inv_vox,
               inv_elems, a_is_prob);
  } else if (nc <= 4) {
    ICL_LAUNCH((icl::loss_grad_kernel<4>), grid, block, 0, st, a, b, lab, stats, weight, gout0, gout1, ga, batch, nc, (long)s, mode, inv_vox,
               inv_elems, a_is_prob);
  } else {
    ICL_LAUNCH((icl::loss_grad_kernel<16>), grid, block, 0, st, a, b, lab, stats, weight, gout0, gout1, ga, batch, nc, (long)s, mode, inv_vox,
               inv_elems, a_is_prob);
  }
  return check_launch("loss_grad");
}

// ---- voxel-wise losses (kernels/loss_point.h): class groups as above — registers for <= 4 and <= 16 classes, the class-walking body for
// 17 .. 256 (or any count under ICL_LOSS_GENERIC=1).  POINT_DISPATCH launches `kern<4 | 16 | 0>` with the arguments behind it.
#define ICL_POINT_DISPATCH(kern, nc, grid, st, ...)                                            \
  do {                                                                                         \
    if ((nc) > 16 || loss_force_generic()) ICL_LAUNCH((icl::kern<0>), grid, dim3(256), 0, st, __VA_ARGS__); \
    else if ((nc) <= 4) ICL_LAUNCH((icl::kern<4>), grid, dim3(256), 0, st, __VA_ARGS__);       \
    else ICL_LAUNCH((icl::kern<16>), grid, dim3(256), 0, st, __VA_ARGS__);                     \
  } while (0)

static int point_loss_shape(const char* who, int64_t outer, int nc, int64_t inner) {
  if (nc < 1 || nc > icl::kLossMaxNc) return fail(-1, "%s: %d classes (1 .. %d)", who, nc, icl::kLossMaxNc);
  if (outer < 1 || inner < 1) return fail(-1, "%s: bad argument", who);
  return 0;
}
static int point_loss_finish(const char* who, hipStream_t st, const float* part, int nblk, float* out, double scale) {
  int rc = check_launch(who);
  if (rc) return rc;
  ICL_LAUNCH(icl::point_finalize_kernel, dim3(1), dim3(256), 0, st, part, nblk, out, scale);
  return check_launch("point_finalize");
}

int icl_kl_fwd(const float* a, const float* b, float* ws, float* out, int64_t outer, int nc, int64_t inner, float w_fwd, float w_rev,
               void* stream) {
  int rc = point_loss_shape("kl_fwd", outer, nc, inner);
  if (rc) return rc;
  if (!a || !b || !ws || !out) return fail(-1, "kl_fwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)outer * inner;
  const int nblk = grid_for(total, 256, ICL_LOSS_MAX_BLOCKS);
  ICL_POINT_DISPATCH(point_kl_fwd_kernel, nc, dim3(nblk), st, a, b, ws, (long)outer, nc, (long)inner, w_fwd, w_rev);
  return point_loss_finish("kl_fwd", st, ws, nblk, out, 1.0 / ((double)total * (double)nc));
}

int icl_kl_bwd(const float* a, const float* b, const float* gout, float* ga, float* gb, int64_t outer, int nc, int64_t inner, float w_fwd,
               float w_rev, void* stream) {
  int rc = point_loss_shape("kl_bwd", outer, nc, inner);
  if (rc) return rc;
  if (!a || !b || !gout || (!ga && !gb)) return fail(-1, "kl_bwd: bad argument");
  const long total = (long)outer * inner;
  ICL_POINT_DISPATCH(point_kl_bwd_kernel, nc, dim3(grid_for(total, 256, 4096)), (hipStream_t)stream, a, b, gout, ga, gb, (long)outer, nc,
                     (long)inner, w_fwd, w_rev, 1.0f / ((float)total * (float)nc));
  return check_launch("kl_bwd");
}

int icl_entropy_fwd(const float* x, float* ws, float* out, float* map, int64_t outer, int nc, int64_t inner, int from_logits, float scale,
                    void* stream) {
  int rc = point_loss_shape("entropy_fwd", outer, nc, inner);
  if (rc) return rc;
  if (!x || (!out && !map)) return fail(-1, "entropy_fwd: bad argument");
  if (out && !ws) return fail(-1, "entropy_fwd: the mean needs the workspace");
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)outer * inner;
  const int nblk = grid_for(total, 256, ICL_LOSS_MAX_BLOCKS);
  ICL_POINT_DISPATCH(point_entropy_fwd_kernel, nc, dim3(nblk), st, x, out ? ws : (float*)nullptr, map, (long)outer, nc, (long)inner, from_logits,
                     scale);
  if (!out) return check_launch("entropy_fwd");
  return point_loss_finish("entropy_fwd", st, ws, nblk, out, (double)scale / (double)total);
}

int icl_entropy_bwd(const float* x, const float* gout, const float* gmap, float* gx, int64_t outer, int nc, int64_t inner, int from_logits,
                    float scale, void* stream) {
  int rc = point_loss_shape("entropy_bwd", outer, nc, inner);
  if (rc) return rc;
  if (!x || !gx || (!gout && !gmap)) return fail(-1, "entropy_bwd: bad argument");
  const long total = (long)outer * inner;
  ICL_POINT_DISPATCH(point_entropy_bwd_kernel, nc, dim3(grid_for(total, 256, 4096)), (hipStream_t)stream, x, gout, gmap, gx, (long)outer, nc,
                     (long)inner, from_logits, scale, 1.0f / (float)total);
  return check_launch("entropy_bwd");
}

int icl_focal_fwd(const float* a, const int64_t* labels, const float* alpha, float* ws, float* out, int64_t outer, int nc, int64_t inner,
                  float gamma, int mean, void* stream) {
  int rc = point_loss_shape("focal_fwd", outer, nc, inner);
  if (rc) return rc;
  if (!a || !labels || !ws || !out || !(gamma >= 0.f)) return fail(-1, "focal_fwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const long total = (long)outer * inner;
  const int nblk = grid_for(total, 256, ICL_LOSS_MAX_BLOCKS);
  ICL_POINT_DISPATCH(point_focal_fwd_kernel, nc, dim3(nblk), st, a, (const long long*)labels, alpha, ws, (long)outer, nc, (long)inner, gamma);
  return point_loss_finish("focal_fwd", st, ws, nblk, out, mean ? 1.0 / (double)total : 1.0);
}

int icl_focal_bwd(const float* a, const int64_t* labels, const float* alpha, const float* gout, float* ga, int64_t outer, int nc,
                  int64_t inner, float gamma, int mean, void* stream) {
  int rc = point_loss_shape("focal_bwd", outer, nc, inner);
  if (rc) return rc;
  if (!a || !labels || !gout || !ga || !(gamma >= 0.f)) return fail(-1, "focal_bwd: bad argument");
  const long total = (long)outer * inner;
  ICL_POINT_DISPATCH(point_focal_bwd_kernel, nc, dim3(grid_for(total, 256, 4096)), (hipStream_t)stream, a, (const long long*)labels, alpha,
                     gout, ga, (long)outer, nc, (long)inner, gamma, mean ? 1.0f / (float)total : 1.0f);
  return check_launch("focal_bwd");
}

int icl_layernorm_fwd(const float* x, const float* gamma, const float* beta, float* y, float* mean, float* rstd, int64_t rows,
                      int c, float eps, void* stream) {
  if (!x || (!gamma != !beta) || !y || !mean || !rstd || rows < 1 || c < 1) return fail(-1, "layernorm_fwd: bad argument");
  constexpr int longrow = 1;
  if (c >= 1024 && c <= 256 * 64 && longrow) {
    // long rows held in registers (bit-identical to the plain kernel, one round of loads instead of three dependent walks)
    if (c <= 256 * 16) ICL_LAUNCH((icl::layernorm_fwd_longrow_kernel<16>), dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y, mean, rstd, c, eps);
    else if (c <= 256 * 32) ICL_LAUNCH((icl::layernorm_fwd_longrow_kernel<32>), dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y, mean, rstd, c, eps);
    else ICL_LAUNCH((icl::layernorm_fwd_longrow_kernel<64>), dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y, mean, rstd, c, eps);
  } else if (c >= 1024) {
    ICL_LAUNCH((icl::layernorm_fwd_kernel<true>), dim3((unsigned)rows), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y, mean, rstd,
               (long)rows, c, eps);
  } else {
    ICL_LAUNCH((icl::layernorm_fwd_kernel<false>), dim3((unsigned)cdivl(rows, 4)), dim3(256), 0, (hipStream_t)stream, x, gamma, beta, y,
               mean, rstd, (long)rows, c, eps);
  }
  return check_launch("layernorm_fwd");
}

namespace {
// row chunks of the LayerNorm parameter-gradient partials: <= 512 chunks of >= 32 rows
long ln_rows_per_chunk(long rows) {
  long rpb = cdivl(rows, 512);
  return rpb < 32 ? 32 : rpb;
}
}  // namespace

int64_t icl_layernorm_bwd_ws_bytes(int64_t rows, int c) {
  if (rows < 1 || c < 1) return 0;
  return (int64_t)2 * cdivl(rows, ln_rows_per_chunk(rows)) * c * 4;
}

int icl_layernorm_bwd(const float* gy, const float* x, const float* gamma, const float* mean, const float* rstd, float* gx,
                      float* dgamma, float* dbeta, void* ws, int64_t rows, int c, void* stream) {
  if (!gy || !x || !mean || !rstd || !gx || ((dgamma || ws) && !gamma) || rows < 1 || c < 1) return fail(-1, "layernorm_bwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  if (!dgamma != !dbeta) return fail(-1, "layernorm_bwd: dgamma and dbeta go together");
  if (dgamma && !ws) return fail(-1, "layernorm_bwd: parameter gradients need the workspace of icl_layernorm_bwd_ws_bytes");
  const long rpb = ln_rows_per_chunk(rows);
  const int chunks = (int)cdivl(rows, rpb);
  float* part_g = (float*)ws;
  float* part_b = part_g ? part_g + (long)chunks * c : nullptr;
  constexpr int fuse_on = 1;
  if (c < 1024 && ws && fuse_on) {
    // rows of one wave: the input gradient and the chunk partials of dgamma / dbeta in ONE launch
    const dim3 grid((unsigned)chunks);
#define ICL_LN_BW(CPL, RU) \
  ICL_LAUNCH((icl::layernorm_bwd_wgrad_kernel<CPL, RU>), grid, dim3(256), 0, st, gy, x, gamma, mean, rstd, gx, part_g, part_b, (long)rows, c, rpb)
    if (c <= 64) ICL_LN_BW(1, 4);
    else if (c <= 128) ICL_LN_BW(2, 4);
    else if (c <= 256) ICL_LN_BW(4, 2);
    else if (c <= 512) ICL_LN_BW(8, 1);
    else ICL_LN_BW(16, 1);
#undef ICL_LN_BW
    int rc = check_launch("layernorm_bwd_wgrad");
    if (rc || !dgamma) return rc;
    const void* g[2] = {part_g, part_b};
    void* out[2] = {dgamma, dbeta};
    const int32_t rr[2] = {chunks, chunks}, cc[2] = {c, c};
    return icl_colsum_multi(g, out, rr, cc, 2, stream);
  }
  constexpr int longrow = 1;
  if (c >= 1024 && c <= 256 * 64 && longrow) {
    if (c <= 256 * 16) ICL_LAUNCH((icl::layernorm_bwd_longrow_kernel<16>), dim3((unsigned)rows), dim3(256), 0, st, gy, x, gamma, mean, rstd, gx, c);
    else if (c <= 256 * 32) ICL_LAUNCH((icl::layernorm_bwd_longrow_kernel<32>), dim3((unsigned)rows), dim3(256), 0, st, gy, x, gamma, mean, rstd, gx, c);
    else ICL_LAUNCH((icl::layernorm_bwd_longrow_kernel<64>), dim3((unsigned)rows), dim3(256), 0, st, gy, x, gamma, mean, rstd, gx, c);
  } else if (c >= 1024) {
    ICL_LAUNCH((icl::layernorm_bwd_kernel<true>), dim3((unsigned)rows), dim3(256), 0, st, gy, x, gamma, mean, rstd, gx, (long)rows, c);
  } else {
    ICL_LAUNCH((icl::layernorm_bwd_kernel<false>), dim3((unsigned)cdivl(rows, 4)), dim3(256), 0, st, gy, x, gamma, mean, rstd, gx,
               (long)rows, c);
  }
  int rc = check_launch("layernorm_bwd");
  if (rc || !ws) return rc;
  int cols = 256;
  while (cols > c && cols > 16) cols >>= 1;  // power of two >= min(c, 256) ... rows of 64 floats use 4 row lanes
  if (cols < c && cols < 256) cols <<= 1;
  ICL_LAUNCH(icl::layernorm_wgrad_kernel, dim3((c + cols - 1) / cols, (unsigned)chunks), dim3(256), 0, st, gy, x, mean, rstd, part_g, part_b,
             (long)rows, c, rpb, cols);
  rc = check_launch("layernorm_wgrad");
  if (rc || !dgamma) return rc;      // ws only: the caller sums the chunk partials (icl_colsum_multi over [chunks][c] twice)
  const void* g[2] = {part_g, part_b};
  void* out[2] = {dgamma, dbeta};
  const int32_t rr[2] = {chunks, chunks}, cc[2] = {c, c};
  return icl_colsum_multi(g, out, rr, cc, 2, stream);
}

int icl_gelu_fwd(const float* x, float* y, int64_t n, void* stream) {
  if (!x || !y || n < 1) return fail(-1, "gelu_fwd: bad argument");
  ICL_LAUNCH(icl::gelu_fwd_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, x, y, (long)n);
  return check_launch("gelu_fwd");
}

int icl_gelu_bwd(const float* gy, const float* x, float* gx, int64_t n, void* stream) {
  if (!gy || !x || !gx || n < 1) return fail(-1, "gelu_bwd: bad argument");
  ICL_LAUNCH(icl::gelu_bwd_kernel, dim3(grid_for(n, 256)), dim3(256), 0, (hipStream_t)stream, gy, x, gx, (long)n);
  return check_launch("gelu_bwd");
}

// more classes than the LDS arrays of the logits and dK / dV kernels hold: the class-tiled instantiations (test-only override ICL_ATTN_TILED=1:
// for any class count, read per call)
static bool attn_class_tiles(int nc) {
  const char* e = getenv("ICL_ATTN_TILED");
  return nc > icl::kAttnMaxNc || (e && atoi(e) == 1);
}

int icl_attn_fwd(const float* q, const float* kv, float* logits, float* out, float* stats, int b, int h, int nc, int n, int d,
                 float scale, void* stream) {
  if (nc < 1 || nc > icl::kAttnMaxClasses) return fail(-1, "attn_fwd: %d classes (1 .. %d)", nc, icl::kAttnMaxClasses);
  if (!q || !kv || !logits || !out || !stats || b < 1 || h < 1 || n < 1 || (d != 8 && d != 16))
    return fail(-1, "attn_fwd: bad argument (head dim 8 or 16)");
  hipStream_t st = (hipStream_t)stream;
  const dim3 g1((n + 255) / 256, b * h), g2(b * h * nc);
  const bool tiled = attn_class_tiles(nc);
  if (d == 16) {
    if (tiled) ICL_LAUNCH((icl::attn_logits_kernel<16, true>), g1, dim3(256), 0, st, q, kv, logits, b, h, nc, n, scale);
    else ICL_LAUNCH((icl::attn_logits_kernel<16, false>), g1, dim3(256), 0, st, q, kv, logits, b, h, nc, n, scale);
    ICL_LAUNCH((icl::attn_softmax_pv_kernel<16, 256>), g2, dim3(256), 0, st, (const float*)logits, kv, out, stats, b, h, nc, n);
  } else {
    if (tiled) ICL_LAUNCH((icl::attn_logits_kernel<8, true>), g1, dim3(256), 0, st, q, kv, logits, b, h, nc, n, scale);
    else ICL_LAUNCH((icl::attn_logits_kernel<8, false>), g1, dim3(256), 0, st, q, kv, logits, b, h, nc, n, scale);
    ICL_LAUNCH((icl::attn_softmax_pv_kernel<8, 256>), g2, dim3(256), 0, st, (const float*)logits, kv, out, stats, b, h, nc, n);
  }
  return check_launch("attn_fwd");
}

int64_t icl_attn_bwd_ws_bytes(int b, int h, int nc, int n, int d) {
  if (b < 1 || h < 1 || nc < 1 || n < 1 || d < 1) return 0;
  return (int64_t)((n + 255) / 256) * b * h * nc * d * 4;
}

int icl_attn_bwd(const float* q, const float* kv, const float* logits, const float* stats, const float* out, const float* gout,
                 const float* glog, float* gq, float* gkv, int b, int h, int nc, int n, int d, float scale, void* stream) {
  return icl_attn_bwd_ws(q, kv, logits, stats, out, gout, glog, gq, gkv, nullptr, b, h, nc, n, d, scale, stream);
}

// ws (icl_attn_bwd_ws_bytes) given: dQ from the per-token-chunk shares the dK / dV pass writes (kernels/token.h), summed in chunk order;
// NULL: the row-per-workgroup dQ kernel
int icl_attn_bwd_ws(const float* q, const float* kv, const float* logits, const float* stats, const float* out, const float* gout,
                    const float* glog, float* gq, float* gkv, void* ws, int b, int h, int nc, int n, int d, float scale, void* stream) {
  if (nc < 1 || nc > icl::kAttnMaxClasses) return fail(-1, "attn_bwd: %d classes (1 .. %d)", nc, icl::kAttnMaxClasses);
  if (!q || !kv || !logits || !stats || !out || !gq || !gkv || b < 1 || h < 1 || n < 1 || (d != 8 && d != 16))
    return fail(-1, "attn_bwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const dim3 g1((n + 255) / 256, b * h), g2(b * h * nc);
  float* pq = (float*)ws;
  const bool tiled = attn_class_tiles(nc);
  if (d == 16) {
    if (tiled) ICL_LAUNCH((icl::attn_bwd_kv_kernel<16, true>), g1, dim3(256), 0, st, q, kv, logits, stats, out, gout, glog, gkv, b, h, nc, n, scale, pq);
    else ICL_LAUNCH((icl::attn_bwd_kv_kernel<16, false>), g1, dim3(256), 0, st, q, kv, logits, stats, out, gout, glog, gkv, b, h, nc, n, scale, pq);
    if (!pq) ICL_LAUNCH((icl::attn_bwd_q_kernel<16, 256>), g2, dim3(256), 0, st, kv, logits, stats, out, gout, glog, gq, b, h, nc, n, scale);
  } else {
    if (tiled) ICL_LAUNCH((icl::attn_bwd_kv_kernel<8, true>), g1, dim3(256), 0, st, q, kv, logits, stats, out, gout, glog, gkv, b, h, nc, n, scale, pq);
    else ICL_LAUNCH((icl::attn_bwd_kv_kernel<8, false>), g1, dim3(256), 0, st, q, kv, logits, stats, out, gout, glog, gkv, b, h, nc, n, scale, pq);
    if (!pq) ICL_LAUNCH((icl::attn_bwd_q_kernel<8, 256>), g2, dim3(256), 0, st, kv, logits, stats, out, gout, glog, gq, b, h, nc, n, scale);
  }
  if (pq) {
    const int rd = b * h * nc * d;
    ICL_LAUNCH(icl::attn_dq_reduce_kernel, dim3((rd + 255) / 256), dim3(256), 0, st, (const float*)pq, gq, (int)g1.x, rd, scale);
  }
  return check_launch("attn_bwd");
}

int64_t icl_window_attn_bias_elems(int n, int heads) { return icl_window_attn_bias_elems_impl(n, heads); }

// ---- Linear weight gradient for tall activations ------------------------------------------------------------------
static int linear_wgrad_nsplit(int64_t rows, int o, int i) {
  // slab traffic (nsplit * O*I) should stay below the activation traffic (rows * (O+I)); enough waves to fill the chip
  const int ob = (o + icl::kLwB - 1) / icl::kLwB, ib = (i + icl::kLwB - 1) / icl::kLwB;
  long n = rows * (o + i) / ((long)o * i + o);
  const long want = (2048 + ob * ib - 1) / (ob * ib);
  if (n > want) n = want;
  const long steps = (rows + 3) / 4;
  if (n > steps / 8) n = steps / 8;   // at least 32 rows per slice
  if (n < 4) n = 4;
  return (int)((n + 3) / 4 * 4);
}

int64_t icl_linear_wgrad_ws_bytes(int64_t rows, int o, int i) {
  return (int64_t)linear_wgrad_nsplit(rows, o, i) * ((int64_t)o * i + o) * 4;
}

int icl_linear_wgrad(const float* gy, const float* x, float* dw, float* db, void* ws, int64_t rows, int o, int i, void* stream) {
  if (!gy || !x || !dw || !ws || rows < 1 || o < 1 || i < 1) return fail(-1, "linear_wgrad: bad argument");
  hipStream_t st = (hipStream_t)stream;
  const int nsplit = linear_wgrad_nsplit(rows, o, i);
  const int ob = (o + icl::kLwB - 1) / icl::kLwB, ib = (i + icl::kLwB - 1) / icl::kLwB;
  ICL_LAUNCH(icl::linear_wgrad_kernel, dim3(nsplit / 4, ob, ib), dim3(256), 0, st, gy, x, (float*)ws, (long)rows, o, i, nsplit);
  if (int rc = check_launch("linear_wgrad")) return rc;
  const long EW = (long)o * i, E = EW + o;
  ICL_LAUNCH(icl::linear_wgrad_reduce_kernel, dim3((unsigned)cdivl(E, 16)), dim3(256), 0, st, (const float*)ws, dw, db, E, EW, nsplit);
  return check_launch("linear_wgrad_reduce");
}

// ---- first convolution of the backbones: one input channel (kernels/conv_cin1.h)
static bool cin1_geom(icl::Cin1Geom& g, int n, int cout, int d, int h, int w, int64_t xbs, int64_t ybs) {
  if (n < 1 || cout < 1 || cout > 16 || d < 1 || h < 1 || w < 1 || (long)d * h * w * 16 >= (1L << 31)) return false;
  g.N = n; g.Cout = cout; g.D = d; g.H = h; g.W = w; g.nty = (h + icl::kC1Rows - 1) / icl::kC1Rows;
  g.x_bstride = xbs; g.y_bstride = ybs; g.ntiles = n * d * g.nty;
  return (size_t)3 * (icl::kC1Rows + 2) * (w + 2) * 4 <= 64 * 1024;
}
// many small workgroups (12 KB of LDS, 4 waves): eight per CU hide the halo staging of one behind the products of the others
static int cin1_grid(const icl::Cin1Geom& g) { return g.ntiles < 2048 ? g.ntiles : 2048; }
static size_t cin1_lds(const icl::Cin1Geom& g) {
  const size_t halo = (size_t)3 * (icl::kC1Rows + 2) * (g.W + 2) * 4;
  return halo > 2048 * 4 ? halo : 2048 * 4;
}

int icl_conv3d_cin1_fwd(const float* x, const float* w, const float* bias, float* y, int n, int cout, int d, int h, int wd, int64_t x_bstride,
                        int64_t y_bstride, void* stream) {
  icl::Cin1Geom g;
  if (!x || !w || !y || !cin1_geom(g, n, cout, d, h, wd, x_bstride, y_bstride)) return fail(-1, "conv3d_cin1_fwd: bad argument");
  ICL_LAUNCH(icl::conv_cin1_fwd_kernel, dim3(cin1_grid(g)), dim3(icl::kC1Threads), cin1_lds(g), (hipStream_t)stream, x, w, bias, y, g);
  snprintf(g_kernel, sizeof(g_kernel), "conv_cin1_fwd_kernel");
  return check_launch("conv3d_cin1_fwd");
}

int64_t icl_conv3d_cin1_wgrad_ws_bytes(int n, int d, int h) {
  const long tiles = (long)n * d * ((h + icl::kC1Rows - 1) / icl::kC1Rows);
  return (tiles < 2048 ? tiles : 2048) * 512 * 4;
}

int icl_conv3d_cin1_wgrad(const float* x, const float* gy, float* gw, void* ws, int n, int cout, int d, int h, int wd, int64_t x_bstride,
                          int64_t gy_bstride, void* stream) {
  icl::Cin1Geom g;
  if (!x || !gy || !gw || !ws || (wd & 3) || (gy_bstride & 3) || !aligned16(gy) || !cin1_geom(g, n, cout, d, h, wd, x_bstride, gy_bstride))
    return fail(-1, "conv3d_cin1_wgrad: bad argument (W and the sample stride of dY must be multiples of 4, dY 16-byte aligned)");
  const int grid = cin1_grid(g);
  ICL_LAUNCH(icl::conv_cin1_wgrad_kernel, dim3(grid), dim3(icl::kC1Threads), cin1_lds(g), (hipStream_t)stream, x, gy, (float*)ws, g);
  if (int rc = check_launch("conv3d_cin1_wgrad")) return rc;
  ICL_LAUNCH(icl::conv_cin1_wgrad_reduce_kernel, dim3(16), dim3(256), 0, (hipStream_t)stream, (const float*)ws, gw, grid, cout);
  snprintf(g_kernel, sizeof(g_kernel), "conv_cin1_wgrad_kernel");
  return check_launch("conv3d_cin1_wgrad_reduce");
}

int64_t icl_conv1x1_wgrad_ws_bytes(int n, int64_t s, int cin, int cout) { return icl_linear_wgrad_ws_bytes((int64_t)n * s, cout, cin); }

namespace {
int conv1x1_wgrad_run(const float* x, const float* gy, float* gw, float* gbias, void* ws, int n, int cin, int cout, int64_t s,
                      int64_t x_bstride, int64_t gy_bstride, const icl::DropSpec& dr, hipStream_t st) {
  const int nsplit = linear_wgrad_nsplit((int64_t)n * s, cout, cin);
  const int ob = (cout + icl::kLwB - 1) / icl::kLwB, ib = (cin + icl::kLwB - 1) / icl::kLwB;
  ICL_LAUNCH(icl::conv1x1_wgrad_kernel, dim3(nsplit / 4, ob, ib), dim3(256), 0, st, gy, x, (float*)ws, n, (long)s, cout, cin, nsplit,
             (long)gy_bstride, (long)x_bstride, dr);
  if (int rc = check_launch("conv1x1_wgrad")) return rc;
  const long EW = (long)cout * cin, E = EW + cout;
  ICL_LAUNCH(icl::linear_wgrad_reduce_kernel, dim3((unsigned)cdivl(E, 16)), dim3(256), 0, st, (const float*)ws, gw, gbias, E, EW, nsplit);
  return check_launch("conv1x1_wgrad_reduce");
}
}  // namespace

int icl_conv1x1_wgrad(const float* x, const float* gy, float* gw, float* gbias, void* ws, int n, int cin, int cout, int64_t s,
                      int64_t x_bstride, int64_t gy_bstride, void* stream) {
  if (!x || !gy || !gw || !ws || n < 1 || cin < 1 || cout < 1 || s < 4 || (s & 3) || (x_bstride & 3) || (gy_bstride & 3))
    return fail(-1, "conv1x1_wgrad: bad argument (voxel count and batch strides must be multiples of 4)");
  return conv1x1_wgrad_run(x, gy, gw, gbias, ws, n, cin, cout, s, x_bstride, gy_bstride, icl::DropSpec{}, (hipStream_t)stream);
}

// ... with x = dropout(x0) given as x0 and the mask's (seed, p): the weight gradient of conv(dropout(x0)); x0 contiguous [n, cin, s]
int icl_conv1x1_wgrad_dropout(const float* x, const float* gy, float* gw, float* gbias, void* ws, int n, int cin, int cout, int64_t s,
                              int64_t gy_bstride, uint32_t seed, float p, const uint32_t* seed_dev, void* stream) {
  if (!x || !gy || !gw || !ws || n < 1 || cin < 1 || cout < 1 || s < 4 || (s & 3) || (gy_bstride & 3) || !(p >= 0.f && p < 1.f))
    return fail(-1, "conv1x1_wgrad_dropout: bad argument");
  return conv1x1_wgrad_run(x, gy, gw, gbias, ws, n, cin, cout, s, (int64_t)cin * s, gy_bstride, drop_spec(1, seed, p, seed_dev), (hipStream_t)stream);
}

// ... with x0 itself given raw + (scale, shift): the weight gradient of conv1x1(dropout(relu(fma(x0, scale, shift)), p))
int icl_conv1x1_wgrad_dropout_norm(const float* x, const float* ss, const float* gy, float* gw, float* gbias, void* ws, int n, int cin, int cout,
                                   int64_t s, int64_t gy_bstride, uint32_t seed, float p, const uint32_t* seed_dev, void* stream) {
  if (!x || !ss || !gy || !gw || !ws || n < 1 || cin < 1 || cout < 1 || s < 4 || (s & 3) || (gy_bstride & 3) || !(p >= 0.f && p < 1.f))
    return fail(-1, "conv1x1_wgrad_dropout_norm: bad argument");
  icl::DropSpec dr = p > 0.f ? drop_spec(1, seed, p, seed_dev) : icl::DropSpec{};
  dr.ss = ss;
  return conv1x1_wgrad_run(x, gy, gw, gbias, ws, n, cin, cout, s, (int64_t)cin * s, gy_bstride, dr, (hipStream_t)stream);
}

int icl_relpos_bias_fwd(const float* table, const int64_t* index, float* bias, int n, int heads, int idx_stride, void* stream) {
  if (!table || !index || !bias || n < 1 || n > idx_stride || heads < 1) return fail(-1, "relpos_bias_fwd: bad argument");
  const int npad = (n + 15) / 16 * 16;
  ICL_LAUNCH(icl::relpos_bias_gather_kernel, dim3(grid_for((long)heads * n * npad, 256)), dim3(256), 0, (hipStream_t)stream, table,
             (const long*)index, bias, n, npad, heads, idx_stride);
  return check_launch("relpos_bias_fwd");
}

int icl_window_attn_fwd(const float* qkv, const float* bias, const int32_t* regions, float* out, float* lse, int b_, int n, int heads,
                        int nw, int head_dim, float scale, void* stream) {
  if (!qkv || !bias || !out || !lse) return fail(-1, "window_attn_fwd: null pointer");
  icl::WinAttnGeom g;
  if (int rc = winattn_geom(g, b_, n, heads, nw, head_dim, scale, "window_attn_fwd")) return rc;
  return winattn_fwd_dispatch(qkv, bias, regions, out, lse, g, head_dim, (hipStream_t)stream);
}

int icl_window_attn_bwd(const float* qkv, const float* bias, const int32_t* regions, const float* out, const float* lse,
                        const float* dout, float* dqkv, float* dbias, int b_, int n, int heads, int nw, int head_dim, float scale,
                        void* stream) {
  if (!qkv || !bias || !out || !lse || !dout || !dqkv) return fail(-1, "window_attn_bwd: null pointer");
  icl::WinAttnGeom g;
  if (int rc = winattn_geom(g, b_, n, heads, nw, head_dim, scale, "window_attn_bwd")) return rc;
  return winattn_bwd_dispatch(qkv, bias, regions, out, lse, dout, dqkv, dbias, g, head_dim, (hipStream_t)stream);
}

// WindowAttention.attn_drop (swinunetr_icl.py:742-747) inside the fused kernels: the same dispatch with the dropout instantiations.
int icl_window_attn_fwd_drop(const float* qkv, const float* bias, const int32_t* regions, float* out, float* lse, int b_, int n, int heads,
                             int nw, int head_dim, float scale, uint32_t seed, float p, const uint32_t* seed_dev, void* stream) {
  if (!qkv || !bias || !out || !lse) return fail(-1, "window_attn_fwd_drop: null pointer");
  icl::WinAttnGeom g;
  icl::WaDrop d;
  if (int rc = winattn_geom(g, b_, n, heads, nw, head_dim, scale, "window_attn_fwd_drop")) return rc;
  if (int rc = winattn_drop_spec(d, seed, p, seed_dev, "window_attn_fwd_drop")) return rc;
  return winattn_fwd_dispatch(qkv, bias, regions, out, lse, g, head_dim, (hipStream_t)stream, d);
}

int icl_window_attn_bwd_drop(const float* qkv, const float* bias, const int32_t* regions, const float* out, const float* lse,
                             const float* dout, float* dqkv, float* dbias, int b_, int n, int heads, int nw, int head_dim, float scale,
                             uint32_t seed, float p, const uint32_t* seed_dev, void* stream) {
  if (!qkv || !bias || !out || !lse || !dout || !dqkv) return fail(-1, "window_attn_bwd_drop: null pointer");
  icl::WinAttnGeom g;
  icl::WaDrop d;
  if (int rc = winattn_geom(g, b_, n, heads, nw, head_dim, scale, "window_attn_bwd_drop")) return rc;
  if (int rc = winattn_drop_spec(d, seed, p, seed_dev, "window_attn_bwd_drop")) return rc;
  return winattn_bwd_dispatch(qkv, bias, regions, out, lse, dout, dqkv, dbias, g, head_dim, (hipStream_t)stream, d);
}

int icl_window_attn_keep_probe(int32_t* out, int64_t base, int count, uint32_t seed, float p, const uint32_t* seed_dev, void* stream) {
  if (!out || count < 1 || base < 0) return fail(-1, "window_attn_keep_probe: bad argument");
  icl::WaDrop d;
  if (int rc = winattn_drop_spec(d, seed, p, seed_dev, "window_attn_keep_probe")) return rc;
  ICL_LAUNCH(icl::window_attn_keep_probe_kernel, dim3(grid_for(count, 256)), dim3(256), 0, (hipStream_t)stream, (int*)out, (long)base, count, d);
  return check_launch("window_attn_keep_probe");
}

int icl_window_attn_bwd_chunks(int b_, int n, int heads, int nw, int head_dim) {
  icl::WinAttnGeom g;
  if (winattn_geom(g, b_, n, heads, nw, head_dim, 1.f, "window_attn_bwd_chunks")) return 0;
  return winattn_bias_chunks(g);
}

int icl_relpos_bias_bwd_sum(float* dbias, int chunks, const int32_t* inv, const int32_t* offs, float* dtable, int64_t table_rows, int n,
                            int heads, void* stream) {
  if (!dbias || !inv || !offs || !dtable || chunks < 1 || n < 1 || heads < 1 || table_rows < 1)
    return fail(-1, "relpos_bias_bwd_sum: bad argument");
  const int npad = (n + 15) / 16 * 16;
  if (chunks > 1) {      // the slices first (coalesced, in order, into slab 0), then one scattered pass over one slab
    const long slab = (long)heads * n * npad;
    ICL_LAUNCH(icl::relpos_bias_slab_sum_kernel, dim3(grid_for(slab / 4, 256, 1024)), dim3(256), 0, (hipStream_t)stream, dbias,
               slab, chunks);
    if (int rc = check_launch("relpos_bias_slab_sum")) return rc;
  }
  ICL_LAUNCH(icl::relpos_bias_gather_sum_kernel, dim3((unsigned)((table_rows + 3) / 4), heads), dim3(256), 0, (hipStream_t)stream, dbias, inv,
             offs, dtable, (int)table_rows, n, npad, heads, 1);
  return check_launch("relpos_bias_bwd_sum");
}

int icl_sgd_step(float* p, const float* g, float* m, int64_t n, float lr, float momentum, float weight_decay, int first,
                 const float* lr_dev, void* stream) {
  if (!p || !g || !m || n < 1) return fail(-1, "sgd_step: bad argument");
  ICL_LAUNCH(icl::sgd_momentum_kernel, dim3(grid_for((n + 3) / 4, 256, 4096)), dim3(256), 0, (hipStream_t)stream, p, g, m, (long)n, lr,
             momentum, weight_decay, first, lr_dev);
  return check_launch("sgd_step");
}

int64_t icl_sgd_factored_split_ws_bytes(int rows, int n, int k) {
  if (rows < 1 || n < 1 || k < 1) return 0;
  return (int64_t)3 * ((rows + 7) / 8) * ((int64_t)n + k) * 16;
}

int icl_sgd_step_factored_split(float* p, float* m, const float* g, const float* x, void* ws, int rows, int n, int k, float lr,
                                float momentum, float weight_decay, int first, const float* lr_dev, void* stream) {
  if (!p || !m || !g || !x || !ws || rows < 1 || n < 1 || k < 4 || (k & 3) || !aligned16(ws))
    return fail(-1, "sgd_step_factored_split: bad argument (k %% 4 == 0, workspace of icl_sgd_factored_split_ws_bytes)");
  hipStream_t st = (hipStream_t)stream;
  const int mb = (rows + 7) / 8;
  uint4* gs = (uint4*)ws;
  uint4* xs = gs + (size_t)3 * mb * n;
  ICL_LAUNCH(icl::factor_split_kernel, dim3(grid_for((long)mb * ((long)n + k), 256, 2048)), dim3(256), 0, st, g, x, gs, xs, rows, n, k);
  int rc = check_launch("factor_split");
  if (rc) return rc;
  const size_t lds = (size_t)icl::kSfLdsFloats * 4;
  ICL_SET_MAX_DYN_LDS(icl::sgd_factored_split_kernel, kMaxDynLdsBig);
  ICL_LAUNCH(icl::sgd_factored_split_kernel, dim3((k + icl::kSfCols - 1) / icl::kSfCols, (n + icl::kSfRows - 1) / icl::kSfRows), dim3(256), lds,
             st, p, m, (const uint4*)gs, (const uint4*)xs, rows, n, k, lr, momentum, weight_decay, first, lr_dev);
  return check_launch("sgd_step_factored_split");
}

int icl_sgd_step_factored(float* p, float* m, const float* g, const float* x, int rows, int n, int k, float lr, float momentum,
                          float weight_decay, int first, const float* lr_dev, void* stream) {
  if (!p || !m || !g || !x || rows < 1 || n < 1 || k < 4 || (k & 3)) return fail(-1, "sgd_step_factored: bad argument (k %% 4 == 0)");
  // <= 16 factor rows (one rank, nc = 2): the VALU form streams p / m 8 % faster (no d-tile transposition); from 17 rows on the MFMA
  // form wins (tools/sgd_probe.py: 32 rows 632 us on the VALU form, 64 rows 578 us on the MFMA form)
  if (rows <= 16) {
    constexpr int variant = 2;   // tuning knob
    const dim3 grid((k + icl::kSvCols - 1) / icl::kSvCols, (n + icl::kSvRows - 1) / icl::kSvRows);
    if (variant == 2) {
      ICL_LAUNCH(icl::sgd_factored_small_kernel<2>, grid, dim3(256), 0, (hipStream_t)stream, p, m, g, x, rows, n, k, lr, momentum, weight_decay,
                 first, lr_dev);
    } else if (variant == 1) {
      ICL_LAUNCH(icl::sgd_factored_small_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, p, m, g, x, rows, n, k, lr, momentum, weight_decay,
                 first, lr_dev);
    } else {
      ICL_LAUNCH(icl::sgd_factored_small_kernel<0>, grid, dim3(256), 0, (hipStream_t)stream, p, m, g, x, rows, n, k, lr, momentum, weight_decay,
                 first, lr_dev);
    }
    return check_launch("sgd_step_factored");
  }
  const size_t lds = (size_t)icl::kSfLdsFloats * 4;
  ICL_SET_MAX_DYN_LDS(icl::sgd_factored_kernel, kMaxDynLdsBig);
  ICL_LAUNCH(icl::sgd_factored_kernel, dim3((k + icl::kSfCols - 1) / icl::kSfCols, (n + icl::kSfRows - 1) / icl::kSfRows), dim3(256), lds,
             (hipStream_t)stream, p, m, g, x, rows, n, k, lr, momentum, weight_decay, first, lr_dev);
  return check_launch("sgd_step_factored");
}

int icl_sgd_step_factored_narrow(float* p, float* m, const float* g, const float* x, int rows, int n, int k, float lr, float momentum,
                                 float weight_decay, int first, const float* lr_dev, int workgroups, void* stream) {
  if (!p || !m || !g || !x || rows < 1 || n < 1 || k < 4 || (k & 3) || workgroups < 1) return fail(-1, "sgd_step_factored_narrow: bad argument");
  if (rows > icl::kSnMaxRows) return 1;      // more factor rows than the narrow form holds: the caller uses icl_sgd_step_factored
  const long tiles = (long)((k + icl::kSnCols - 1) / icl::kSnCols) * ((n + icl::kSvRows - 1) / icl::kSvRows);
  const int grid = (int)(tiles < workgroups ? tiles : workgroups);
  const size_t lds = (size_t)icl::kSnMaxRows * (icl::kSnCols / 4) * 16 + (size_t)icl::kSnMaxRows * icl::kSvRows * 4;
  ICL_SET_MAX_DYN_LDS(icl::sgd_factored_narrow_kernel, 96 * 1024);
  ICL_LAUNCH(icl::sgd_factored_narrow_kernel, dim3(grid), dim3(1024), lds, (hipStream_t)stream, p, m, g, x, rows, n, k, lr, momentum, weight_decay,
             first, lr_dev);
  return check_launch("sgd_step_factored_narrow");
}

int icl_sgd_step_multi(void* const* p, const void* const* g, void* const* m, const int64_t* n, int count, float lr,
                       float momentum, float weight_decay, int first, const float* lr_dev, void* stream) {
  if (!p || !g || !m || !n || count < 1) return fail(-1, "sgd_step_multi: bad argument");
  for (int base = 0; base < count; base += icl::kSgdMulti) {
    icl::SgdMulti t{};
    const int k = count - base < icl::kSgdMulti ? count - base : icl::kSgdMulti;
    long nmax = 1;
    for (int i = 0; i < k; ++i) {
      t.p[i] = (float*)p[base + i];
      t.g[i] = (const float*)g[base + i];
      t.m[i] = (float*)m[base + i];
      t.n[i] = (long)n[base + i];
      if (!t.p[i] || !t.g[i] || !t.m[i] || t.n[i] < 1) return fail(-1, "sgd_step_multi: bad tensor %d", base + i);
      if (t.n[i] > nmax) nmax = t.n[i];
    }
    ICL_LAUNCH(icl::sgd_momentum_multi_kernel, dim3(grid_for((nmax + 3) / 4, 256, 64), k), dim3(256), 0, (hipStream_t)stream, t, lr,
               momentum, weight_decay, first, lr_dev);
    const int rc = check_launch("sgd_step_multi");
    if (rc) return rc;
  }
  return 0;
}

// ---- AdamW (kernels/adamw.h).  Bad arguments launch nothing.
int icl_adamw_step(float* p, const float* g, float* m, float* v, int64_t n, float decay, float step_size, float bc2_sqrt, float beta2,
                   float omb1, float omb2, float eps, int first, const float* hyper_dev, void* stream) {
  if (!p || !g || !m || !v || n < 1) return fail(-1, "adamw_step: bad argument (null pointer or n < 1)");
  const icl::AdamwHyper h{decay, step_size, bc2_sqrt, beta2, omb1, omb2, eps};
  ICL_LAUNCH(icl::adamw_kernel, dim3(grid_for((n + 3) / 4, 256, 4096)), dim3(256), 0, (hipStream_t)stream, p, g, m, v, (long)n, h, first,
             hyper_dev);
  return check_launch("adamw_step");
}

int icl_adamw_step_multi(void* const* p, const void* const* g, void* const* m, void* const* v, const int64_t* n, int count, float decay,
                         float step_size, float bc2_sqrt, float beta2, float omb1, float omb2, float eps, int first,
                         const float* hyper_dev, void* stream) {
  if (!p || !g || !m || !v || !n || count < 1) return fail(-1, "adamw_step_multi: bad argument");
  for (int i = 0; i < count; ++i)      // the whole list is checked before the first launch: a bad entry leaves every tensor untouched
    if (!p[i] || !g[i] || !m[i] || !v[i] || n[i] < 1) return fail(-1, "adamw_step_multi: bad tensor %d (null pointer or n < 1)", i);
  const icl::AdamwHyper h{decay, step_size, bc2_sqrt, beta2, omb1, omb2, eps};
  for (int base = 0; base < count; base += icl::kAdamwMulti) {
    icl::AdamwMulti t{};
    const int k = count - base < icl::kAdamwMulti ? count - base : icl::kAdamwMulti;
    long nmax = 1;
    for (int i = 0; i < k; ++i) {
      t.p[i] = (float*)p[base + i];
      t.g[i] = (const float*)g[base + i];
      t.m[i] = (float*)m[base + i];
      t.v[i] = (float*)v[base + i];
      t.n[i] = (long)n[base + i];
      if (t.n[i] > nmax) nmax = t.n[i];
    }
    ICL_LAUNCH(icl::adamw_multi_kernel, dim3(grid_for((nmax + 3) / 4, 256, 64), k), dim3(256), 0, (hipStream_t)stream, t, h, first, hyper_dev);
    const int rc = check_launch("adamw_step_multi");
    if (rc) return rc;
  }
  return 0;
}

int icl_adamw_step_factored(float* p, float* m, float* v, const float* g, const float* x, int rows, int n, int k, float decay,
                            float step_size, float bc2_sqrt, float beta2, float omb1, float omb2, float eps, int first,
                            const float* hyper_dev, void* stream) {
  if (!p || !m || !v || !g || !x || rows < 1 || n < 1 || k < 4 || (k & 3))
    return fail(-1, "adamw_step_factored: bad argument (null pointer, rows < 1, n < 1 or k %% 4 != 0)");
  if (!aligned16(p) || !aligned16(m) || !aligned16(v) || !aligned16(x)) return fail(-1, "adamw_step_factored: p, m, v and x need 16-byte alignment");
  const icl::AdamwHyper h{decay, step_size, bc2_sqrt, beta2, omb1, omb2, eps};
  const dim3 grid((k + icl::kAvCols - 1) / icl::kAvCols, (n + icl::kAvRows - 1) / icl::kAvRows);
  ICL_LAUNCH(icl::adamw_factored_kernel, grid, dim3(256), 0, (hipStream_t)stream, p, m, v, g, x, rows, n, k, h, first, hyper_dev);
  return check_launch("adamw_step_factored");
}

// ---- gradient clipping by the global 2-norm (kernels/gradclip.h).  Bad arguments launch nothing.
namespace {
struct GcGramPlan { int pairs, slab_g, slab_x, nslab_g, nslab_x; };
constexpr int kGcMaxRows = 1024, kGcMaxChunks = 4096;

// slabs of the long axes: whole 128-column pieces, about 256 workgroups per side over all pairs of row chunks and at most 64 slabs (the
// combine kernel walks an entry's slabs in one thread; tools/gradclip_probe.py: with 108 slabs that walk was the whole cost at 8 rows)
GcGramPlan gc_gram_plan(int rows, int n, int k) {
  GcGramPlan p;
  const int nch = (rows + icl::kGcRows - 1) / icl::kGcRows;
  p.pairs = nch * (nch + 1) / 2;
  const int target = 256 / p.pairs > 64 ? 64 : (256 / p.pairs < 4 ? 4 : 256 / p.pairs);
  p.slab_g = round_up((int)cdivl(n, target), icl::kGcCols);
  p.slab_x = round_up((int)cdivl(k, target), icl::kGcCols);
  p.nslab_g = (int)cdivl(n, p.slab_g);
  p.nslab_x = (int)cdivl(k, p.slab_x);
  return p;
}
}  // namespace

int64_t icl_gradclip_factored_ws_bytes(int rows, int n, int k) {
  if (rows < 1 || rows > kGcMaxRows || n < 1 || k < 1) return 0;
  const GcGramPlan p = gc_gram_plan(rows, n, k);
  return (int64_t)(p.nslab_g + p.nslab_x) * rows * rows * 8;
}

int icl_gradclip_factored_parts(int rows) { return rows < 1 || rows > kGcMaxRows ? 0 : (rows * rows + 255) / 256; }

int icl_gradclip_sumsq(const void* const* g, const int64_t* n, int count, int chunks, double* partial, void* stream) {
  if (!g || !n || !partial || count < 1 || chunks < 1 || chunks > kGcMaxChunks || ((uintptr_t)partial & 7))
    return fail(-1, "gradclip_sumsq: bad argument (null pointer, count < 1, chunks outside 1..%d or partial not 8-byte aligned)", kGcMaxChunks);
  for (int i = 0; i < count; ++i)      // the whole list is checked before the first launch
    if (!g[i] || n[i] < 1) return fail(-1, "gradclip_sumsq: bad tensor %d (null pointer or n < 1)", i);
  for (int base = 0; base < count; base += icl::kGcMulti) {
    icl::GcSumsqMulti t{};
    const int k = count - base < icl::kGcMulti ? count - base : icl::kGcMulti;
    for (int i = 0; i < k; ++i) {
      t.g[i] = (const float*)g[base + i];
      t.n[i] = (long)n[base + i];
    }
    ICL_LAUNCH(icl::gradclip_sumsq_multi_kernel, dim3(chunks, k), dim3(256), 0, (hipStream_t)stream, t, partial + (long)base * chunks);
    const int rc = check_launch("gradclip_sumsq");
    if (rc) return rc;
  }
  return 0;
}

int icl_gradclip_sumsq_factored(const float* g, const float* x, int rows, int n, int k, void* ws, double* partial, void* stream) {
  if (!g || !x || !ws || !partial || rows < 1 || rows > kGcMaxRows || n < 1 || k < 1 || ((uintptr_t)ws & 7) || ((uintptr_t)partial & 7))
    return fail(-1, "gradclip_sumsq_factored: bad argument (null pointer, rows outside 1..%d, n < 1, k < 1 or ws / partial not 8-byte aligned)",
                kGcMaxRows);
  const GcGramPlan p = gc_gram_plan(rows, n, k);
  const int nslab = p.nslab_g > p.nslab_x ? p.nslab_g : p.nslab_x;
  ICL_LAUNCH(icl::gradclip_gram_kernel, dim3(nslab, p.pairs, 2), dim3(256), 0, (hipStream_t)stream, g, x, rows, n, k, p.slab_g, p.slab_x,
             p.nslab_g, p.nslab_x, (double*)ws);
  int rc = check_launch("gradclip_sumsq_factored");
  if (rc) return rc;
  ICL_LAUNCH(icl::gradclip_gram_combine_kernel, dim3(icl_gradclip_factored_parts(rows)), dim3(256), 0, (hipStream_t)stream, (const double*)ws,
             rows, p.nslab_g, p.nslab_x, partial);
  return check_launch("gradclip_sumsq_factored");
}

int icl_gradclip_finish(const double* partial, int64_t count, float max_norm, float* clip_dev, void* stream) {
  if (!partial || !clip_dev || count < 1 || ((uintptr_t)partial & 7))
    return fail(-1, "gradclip_finish: bad argument (null pointer, count < 1 or partial not 8-byte aligned)");
  ICL_LAUNCH(icl::gradclip_finish_kernel, dim3(1), dim3(256), 0, (hipStream_t)stream, partial, (long)count, max_norm, clip_dev);
  return check_launch("gradclip_finish");
}

int icl_gradclip_scale(void* const* dst, const void* const* src, const int64_t* n, int count, int chunks, const float* clip_dev,
                       void* stream) {
  if (!dst || !src || !n || !clip_dev || count < 1 || chunks < 1 || chunks > kGcMaxChunks)
    return fail(-1, "gradclip_scale: bad argument (null pointer, count < 1 or chunks outside 1..%d)", kGcMaxChunks);
  for (int i = 0; i < count; ++i)
    if (!dst[i] || !src[i] || n[i] < 1) return fail(-1, "gradclip_scale: bad tensor %d (null pointer or n < 1)", i);
  for (int base = 0; base < count; base += icl::kGcMulti) {
    icl::GcScaleMulti t{};
    const int k = count - base < icl::kGcMulti ? count - base : icl::kGcMulti;
    for (int i = 0; i < k; ++i) {
      t.dst[i] = (float*)dst[base + i];
      t.src[i] = (const float*)src[base + i];
      t.n[i] = (long)n[base + i];
    }
    ICL_LAUNCH(icl::gradclip_scale_multi_kernel, dim3(chunks, k), dim3(256), 0, (hipStream_t)stream, t, clip_dev);
    const int rc = check_launch("gradclip_scale");
    if (rc) return rc;
  }
  return 0;
}

int64_t icl_gemm_ws_bytes(int64_t m, int n, int k, int batch) { return gemm_ws_bytes_impl((long)m, n, k, batch < 1 ? 1 : batch); }

int icl_gemm(const float* a, const float* b, float* c, const float* bias, void* ws, int64_t m, int n, int k, int64_t lda, int64_t ldb,
             int64_t ldc, int a_kcontig, int b_kcontig, int act, int batch, int64_t a_bstride, int64_t b_bstride, int64_t c_bstride,
             void* stream) {
  if (!a || !b || !c || m < 1 || n < 1 || k < 1 || batch < 1 || m > 0x7fffffff) return fail(-1, "gemm: bad argument");
  return gemm_run(a, b, c, bias, ws, (long)m, n, k, (long)lda, (long)ldb, (long)ldc, a_kcontig, b_kcontig, act, batch, (long)a_bstride,
                  (long)b_bstride, (long)c_bstride, (hipStream_t)stream);
}

int64_t icl_linear_ws_bytes(int64_t rows, int in, int out, int kind) {
  if (kind == 0) return linear_streams(rows, in, out) ? stream_ws_bytes((long)rows, in, out, false) : gemm_ws_bytes_impl((long)rows, out, in, 1);
  if (kind == 1) return linear_streams(rows, in, out) ? stream_ws_bytes((long)rows, in, out, true) : gemm_ws_bytes_impl((long)rows, in, out, 1);
  if (kind == 3) {                                          // fused input gradient + SGD update: the slabs of the streaming plan
    const StreamPlan p = stream_plan((long)rows, in, out, true);
    return (int64_t)p.nslice * 16 * p.mt * in * 4;
  }
  if (rows <= 32 && (in & 3) == 0) return 0;              // kind 2: weight gradient dW[out][in] = gy^T x (few rows: outer products)
  return gemm_ws_bytes_impl(out, in, (int)rows, 1);
}

int icl_linear_fwd(const float* x, const float* w, const float* bias, float* y, void* ws, int64_t rows, int in, int out, int act,
                   void* stream) {
  if (!x || !w || !y || rows < 1 || in < 1 || out < 1 || rows > 0x7fffffff) return fail(-1, "linear_fwd: bad argument");
  hipStream_t st = (hipStream_t)stream;
  if (linear_streams(rows, in, out) && aligned16(x) && aligned16(w) && aligned16(y) && (ws || icl_linear_ws_bytes(rows, in, out, 0) == 0))
    return stream_run(x, w, bias, y, ws, (long)rows, in, out, false, act, st);
  {
    const int rc = linear_rows<false>(x, w, bias, y, (long)rows, in, out, act, st);
    if (rc != 1) return rc;
  }
  return gemm_run(x, w, y, bias, ws, (long)rows, out, in, in, in, out, 1, 1, act, 1, 0, 0, 0, st);
}

int icl_linear_dgrad(const float* gy, const float* w, float* gx, void* ws, int64_t rows, int in, int out, void* stream) {
  if (!gy || !w || !gx || rows < 1 || in < 1 || out < 1 || rows > 0x7fffffff) return fail(-1, "linear_dgrad: bad argument");
  hipStream_t st = (hipStream_t)stream;
  if (linear_streams(rows, in, out) && aligned16(gy) && aligned16(w) && aligned16(gx) && (ws || icl_linear_ws_bytes(rows, in, out, 1) == 0))
    return stream_run(gy, w, nullptr, gx, ws, (long)rows, in, out, true, 0, st);
  {   // gx = gy W with W [out][in]: the weight as [K = out][N = in]
    const int rc = linear_rows<true>(gy, w, nullptr, gx, (long)rows, out, in, 0, st);
    if (rc != 1) return rc;
  }
  return gemm_run(gy, w, gx, nullptr, ws, (long)rows, in, out, out, in, in, 1, 0, 0, 1, 0, 0, 0, st);
}

// gx = gy W and dW = gy^T x of a Linear layer with <= 32 rows in ONE launch (the weight-streaming input-gradient kernel with extra workgroup
// columns for the outer products); returns 1 without launching when the shapes do not take that path (the caller then runs the two calls)
int icl_linear_bwd_small(const float* gy, const float* w, const float* x, float* gx, float* dw, void* ws, int64_t rows, int in, int out,
                         void* stream) {
  if (!gy || !w || !x || !gx || !dw || rows < 1 || in < 1 || out < 1) return fail(-1, "linear_bwd_small: bad argument");
  if (!(rows <= 32 && linear_streams(rows, in, out) && aligned16(gy) && aligned16(w) && aligned16(gx) && aligned16(x) && aligned16(dw) &&
        (ws || icl_linear_ws_bytes(rows, in, out, 1) == 0)))
    return 1;
  if ((long)in * out >= (1L << 24)) return 1;      // big matrices: their weight gradient stays factored / goes its own way
  return stream_run(gy, w, nullptr, gx, ws, (long)rows, in, out, true, 0, (hipStream_t)stream, x, dw);
}

int icl_linear_wgrad_small(const float* gy, const float* x, float* dw, void* ws, int64_t rows, int in, int out, void* stream) {
  if (!gy || !x || !dw || rows < 1 || in < 1 || out < 1 || rows > 0x7fffffff) return fail(-1, "linear_wgrad_small: bad argument");
  if (rows <= 32 && (in & 3) == 0 && aligned16(x) && aligned16(dw)) {   // a handful of outer products: VALU, one launch
    ICL_LAUNCH(icl::linear_wgrad_outer_kernel, dim3(grid_for((long)out * (in / 4), 256, 4096)), dim3(256), 0, (hipStream_t)stream, gy, x, dw,
               (int)rows, out, in);
    return check_launch("linear_wgrad_outer");
  }
  // dW[o][i] = sum_r gy[r][o] x[r][i]: both operands k-strided (k = the row index)
  return gemm_run(gy, x, dw, nullptr, ws, out, in, (int)rows, out, in, in, 0, 0, 0, 1, 0, 0, 0, (hipStream_t)stream);
}

namespace {

// The record of the crop entries from the caller's rows of 11 integers.  Returns -1, or the first sample that is refused (a null
// volume pointer or a value of its row out of range): each entry words its own refusal.
int crop_feed_records(const void* const* images, const void* const* labels, const int32_t* params, int batch, icl::FeedBatch& fb) {
  for (int b = 0; b < batch; ++b) {
    const int32_t* q = params + 11 * b;
    icl::FeedSample& s = fb.s[b];
    s.image = (const float*)images[b];
    s.label = (const uint8_t*)labels[b];
    s.n0 = q[0]; s.n1 = q[1]; s.n2 = q[2]; s.k = q[3]; s.flip_axis = q[4];
    s.p0 = q[5]; s.p1 = q[6]; s.p2 = q[7]; s.c0 = q[8]; s.c1 = q[9]; s.c2 = q[10];
    if (!s.image || !s.label || s.n0 < 1 || s.n1 < 1 || s.n2 < 1 || s.k < 0 || s.k > 3 || s.flip_axis > 1 || s.p0 < 0 || s.p1 < 0 || s.p2 < 0) return b;
  }
  return -1;
}

// Every check of the channel entries icl_crop_rotflip_channels / icl_crop_rotflip_affine (`what`: the entry's name), and their record.
int crop_channels_records(const char* what, const void* const* images, const void* const* labels, const int32_t* params, int batch, int channels,
                          const float* image_out, const int64_t* label_out, int o0, int o1, int o2, icl::FeedBatch& fb) {
  if (!images || !labels || !params || !image_out || !label_out) return fail(-1, "%s: null pointer", what);
  if (batch < 1 || batch > icl::kFeedMaxBatch) return fail(-1, "%s: batch %d out of range (1 <= batch <= %d)", what, batch, icl::kFeedMaxBatch);
  if (channels < 1 || channels > icl::kChannelNormMaxChannels)
    return fail(-1, "%s: channels %d out of range (1 <= channels <= %d)", what, channels, icl::kChannelNormMaxChannels);
  if (o0 < 1 || o1 < 1 || o2 < 1) return fail(-1, "%s: output extents %d x %d x %d (each must be >= 1)", what, o0, o1, o2);
  if ((long)o0 * o1 * o2 > 0x7fffffffL) return fail(-1, "%s: output extents %d x %d x %d (more than 2^31 - 1 voxels a sample)", what, o0, o1, o2);
  const int bad = crop_feed_records(images, labels, params, batch, fb);
  if (bad >= 0 && !(fb.s[bad].image && fb.s[bad].label)) return fail(-1, "%s: sample %d: null volume pointer", what, bad);
  if (bad >= 0) return fail(-1, "%s: bad sample %d", what, bad);
  return 0;
}

// Row b of the affine rows of icl_crop_rotflip_affine / icl_volume_feed_affine[_origins]: flag in {0, 1}, then M row-major, nine finite
// entries with |M_ab| <= 16.
int affine_rows(const char* what, const double* affine_params, int b, int& flag_out, double (&m_out)[9]) {
  const double* q = affine_params + 10 * b;
  if (!(q[0] == 0.0 || q[0] == 1.0)) return fail(-1, "%s: sample %d: affine flag %g (must be 0 or 1)", what, b, q[0]);
  flag_out = q[0] == 1.0 ? 1 : 0;
  for (int e = 0; e < 9; ++e) {
    const double m = q[1 + e];
    if (!std::isfinite(m)) return fail(-1, "%s: sample %d: affine matrix entry M[%d][%d] = %g is not finite", what, b, e / 3, e % 3, m);
    if (std::fabs(m) > 16.0) return fail(-1, "%s: sample %d: affine matrix entry M[%d][%d] = %g outside [-16, 16]", what, b, e / 3, e % 3, m);
    m_out[e] = m;
  }
  return 0;
}

}  // namespace

int icl_crop_rotflip(const void* const* images, const void* const* labels, const int32_t* params, int batch, float* image_out,
                     int64_t* label_out, int o0, int o1, int o2, void* stream) {
  if (!images || !labels || !params || !image_out || !label_out || batch < 1 || batch > icl::kFeedMaxBatch || o0 < 1 || o1 < 1 || o2 < 1)
    return fail(-1, "crop_rotflip: bad argument (1 <= batch <= %d)", icl::kFeedMaxBatch);
  icl::FeedBatch fb{};
  const int bad = crop_feed_records(images, labels, params, batch, fb);
  if (bad >= 0) return fail(-1, "crop_rotflip: bad sample %d", bad);
  ICL_LAUNCH(icl::crop_rotflip_kernel, dim3(grid_for((long)batch * o0 * o1 * o2, 256, 8192)), dim3(256), 0, (hipStream_t)stream, fb, image_out,
             (long long*)label_out, batch, o0, o1, o2);
  return check_launch("crop_rotflip");
}

int icl_crop_rotflip_channels(const void* const* images, const void* const* labels, const int32_t* params, int batch, int channels,
                              float* image_out, int64_t* label_out, int o0, int o1, int o2, void* stream) {
  icl::FeedBatch fb{};
  if (const int rc = crop_channels_records("crop_rotflip_channels", images, labels, params, batch, channels, image_out, label_out, o0, o1, o2, fb))
    return rc;
  const long voxels = (long)o0 * o1 * o2;      // per sample and channel; one grid row per sample
  const int cap = 2048 / batch;                // 2048 workgroups of 256 threads: every wave slot of the 256 CUs once, the rest by stride
  if ((o2 & 3) == 0 && aligned16(image_out) && aligned16(label_out)) {
    ICL_LAUNCH(icl::crop_rotflip_channels_kernel<4>, dim3(grid_for(voxels / 4, 256, cap), batch), dim3(256), 0, (hipStream_t)stream, fb, image_out,
               (long long*)label_out, channels, o0, o1, o2);
  } else {
    ICL_LAUNCH(icl::crop_rotflip_channels_kernel<1>, dim3(grid_for(voxels, 256, cap), batch), dim3(256), 0, (hipStream_t)stream, fb, image_out,
               (long long*)label_out, channels, o0, o1, o2);
  }
  return check_launch("crop_rotflip_channels");
}

int icl_crop_rotflip_affine(const void* const* images, const void* const* labels, const int32_t* params, const double* affine_params, int batch,
                            int channels, float* image_out, int64_t* label_out, int o0, int o1, int o2, void* stream) {
  // a null among the other pointers is refused first, by the shared checks
  if (!affine_params && images && labels && params && image_out && label_out)
    return fail(-1, "crop_rotflip_affine: affine_params is a null pointer");
  icl::FeedBatch fb{};
  if (const int rc = crop_channels_records("crop_rotflip_affine", images, labels, params, batch, channels, image_out, label_out, o0, o1, o2, fb))
    return rc;
  icl::CropAffineBatch ab{};
  bool any = false;
  for (int b = 0; b < batch; ++b) {
    ab.s[b].f = fb.s[b];
    if (const int rc = affine_rows("crop_rotflip_affine", affine_params, b, ab.s[b].affine, ab.s[b].m)) return rc;
    any = any || ab.s[b].affine;
  }
  static_assert(sizeof(icl::CropAffineBatch) == 16 * 144, "16 records of 144 B: 2,304 B of the 4 KB kernel-argument block");
  const long voxels = (long)o0 * o1 * o2;      // per sample and channel; one grid row per sample
  // no affine sample: the grid of icl_crop_rotflip_channels.  Otherwise one thread per output voxel (the affine path's mapping, whatever
  // V), up to 8192 workgroups a sample as for icl_volume_feed_affine; the threads an integer-path sample does not need leave at once
  const int cap = any ? 8192 : 2048 / batch;
  if ((o2 & 3) == 0 && aligned16(image_out) && aligned16(label_out)) {
    ICL_LAUNCH(icl::crop_rotflip_affine_kernel<4>, dim3(grid_for(any ? voxels : voxels / 4, 256, cap), batch), dim3(256), 0, (hipStream_t)stream,
               ab, image_out, (long long*)label_out, channels, o0, o1, o2);
  } else {
    ICL_LAUNCH(icl::crop_rotflip_affine_kernel<1>, dim3(grid_for(voxels, 256, cap), batch), dim3(256), 0, (hipStream_t)stream, ab, image_out,
               (long long*)label_out, channels, o0, o1, o2);
  }
  return check_launch("crop_rotflip_affine");
}

namespace {

int channel_norm_args(const char* what, const float* image, int channels, int64_t voxels, int mask_mode) {
  if (!image) return fail(-1, "%s: null pointer", what);
  if (channels < 1 || channels > icl::kChannelNormMaxChannels)
    return fail(-1, "%s: channels %d out of range (1 <= channels <= %d)", what, channels, icl::kChannelNormMaxChannels);
  if (voxels < 1 || voxels > 0x7fffffffL) return fail(-1, "%s: %lld voxels a channel (must be in 1 .. 2^31 - 1)", what, (long long)voxels);
  if (mask_mode < icl::kNormNonzero || mask_mode > icl::kNormAll)
    return fail(-1, "%s: mask mode %d (0 nonzero, 1 positive, 2 all)", what, mask_mode);
  return 0;
}

}  // namespace

int icl_channel_norm_stats(const float* image, int channels, int64_t voxels, int mask_mode, double* stats_out, double* ws, void* stream) {
  if (!stats_out || !ws) return fail(-1, "channel_norm_stats: null pointer");
  if (const int rc = channel_norm_args("channel_norm_stats", image, channels, voxels, mask_mode)) return rc;
  const int blocks = grid_for(cdivl(voxels, 4), icl::kChannelNormThreads, icl::kChannelNormBlocks);
  const int vec = (voxels & 3) == 0 && aligned16(image) ? 1 : 0;
  const dim3 grid(blocks, channels), block(icl::kChannelNormThreads);
  ICL_LAUNCH(icl::channel_norm_partial_kernel<1>, grid, block, 0, (hipStream_t)stream, image, (long)voxels, mask_mode, vec,
             (const double*)stats_out, ws);
  if (const int rc = check_launch("channel_norm_partial<1>")) return rc;
  ICL_LAUNCH(icl::channel_norm_finish_kernel<1>, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)ws, channels, blocks, stats_out);
  if (const int rc = check_launch("channel_norm_finish<1>")) return rc;
  ICL_LAUNCH(icl::channel_norm_partial_kernel<2>, grid, block, 0, (hipStream_t)stream, image, (long)voxels, mask_mode, vec,
             (const double*)stats_out, ws);
  if (const int rc = check_launch("channel_norm_partial<2>")) return rc;
  ICL_LAUNCH(icl::channel_norm_finish_kernel<2>, dim3(1), dim3(64), 0, (hipStream_t)stream, (const double*)ws, channels, blocks, stats_out);
  return check_launch("channel_norm_finish<2>");
}

int icl_channel_norm_apply(float* image, int channels, int64_t voxels, int mask_mode, int apply_mode, const double* stats, void* stream) {
  if (!stats) return fail(-1, "channel_norm_apply: null pointer");
  if (const int rc = channel_norm_args("channel_norm_apply", image, channels, voxels, mask_mode)) return rc;
  if (apply_mode != 0 && apply_mode != 1) return fail(-1, "channel_norm_apply: apply mode %d (0 mask, 1 all)", apply_mode);
  if ((voxels & 3) == 0 && aligned16(image)) {
    ICL_LAUNCH(icl::channel_norm_apply_kernel<4>, dim3(grid_for(voxels / 4, icl::kChannelNormThreads, 8192), channels),
               dim3(icl::kChannelNormThreads), 0, (hipStream_t)stream, image, (long)voxels, mask_mode, apply_mode, stats);
  } else {
    ICL_LAUNCH(icl::channel_norm_apply_kernel<1>, dim3(grid_for(voxels, icl::kChannelNormThreads, 8192), channels),
               dim3(icl::kChannelNormThreads), 0, (hipStream_t)stream, image, (long)voxels, mask_mode, apply_mode, stats);
  }
  return check_launch("channel_norm_apply");
}

namespace {

// The argument record of icl_volume_feed / icl_volume_feed_origins from the caller's rows, with every check of both.  device_origins:
// the origin fields of the rows are not read; the record's c0, c1, c2 become the largest legal origin n - s (the kernel clamps).
int volume_feed_records(const char* what, const void* const* images, const void* const* labels, const int32_t* int_params,
                        const float* float_params, int batch, int R0, int R1, int R2, bool device_origins, icl::VolumeFeedBatch& fb) {
  if (batch < 1 || batch > icl::kFeedMaxBatch) return fail(-1, "%s: batch %d out of range (1 <= batch <= %d)", what, batch, icl::kFeedMaxBatch);
  if (R0 < 1 || R1 < 1 || R2 < 1) return fail(-1, "%s: output extents %d x %d x %d (each must be >= 1)", what, R0, R1, R2);
  if ((long)R0 * R1 * R2 > 0x7fffffffL) return fail(-1, "%s: output extents %d x %d x %d (more than 2^31 - 1 voxels a sample)", what, R0, R1, R2);
  const int R[3] = {R0, R1, R2};
  for (int b = 0; b < batch; ++b) {
    const int32_t* q = int_params + 14 * b;      // n[3], c[3], s[3], l[3], flip, k
    icl::VolumeFeedSample& s = fb.s[b];
    s.image = (const float*)images[b];
    s.label = (const uint8_t*)labels[b];
    if (!s.image || !s.label) return fail(-1, "%s: sample %d: null volume pointer", what, b);
    for (int a = 0; a < 3; ++a) {
      const int n = q[a], c = q[3 + a], sz = q[6 + a], l = q[9 + a];
      if (n < 1) return fail(-1, "%s: sample %d: extent %d of axis %d (must be >= 1)", what, b, n, a);
      if (device_origins) {
        if (sz < 1 || sz > n) return fail(-1, "%s: sample %d: crop size %d of axis %d outside 1..%d", what, b, sz, a, n);
      } else if (c < 0 || sz < 1 || (long)c + sz > n) {
        return fail(-1, "%s: sample %d: crop [%d, %d + %d) of axis %d outside the extent %d", what, b, c, c, sz, a, n);
      }
      if (l < 0 || (long)l + sz > R[a])
        return fail(-1, "%s: sample %d: left pad %d + crop size %d of axis %d outside the output extent %d", what, b, l, sz, a, R[a]);
    }
    s.n1 = q[1]; s.n2 = q[2];
    s.c0 = q[3]; s.c1 = q[4]; s.c2 = q[5];
    s.s0 = q[6]; s.s1 = q[7]; s.s2 = q[8];
    if (device_origins) { s.c0 = q[0] - s.s0; s.c1 = q[1] - s.s1; s.c2 = q[2] - s.s2; }
    s.l0 = q[9]; s.l1 = q[10]; s.l2 = q[11];
    s.flip = q[12]; s.k = q[13];
    s.mul = float_params[2 * b]; s.add = float_params[2 * b + 1];
    if (s.flip < 0 || s.flip > 7) return fail(-1, "%s: sample %d: flip mask %d outside 0..7", what, b, s.flip);
    if (s.k < 0 || s.k > 3) return fail(-1, "%s: sample %d: k = %d outside 0..3", what, b, s.k);
    if ((s.k & 1) && R0 != R1)
      return fail(-1, "%s: sample %d: k = %d with output extents %d x %d (an odd rot90 needs R0 == R1)", what, b, s.k, R0, R1);
  }
  return 0;
}

extern "C++" template <int V, bool DEV, typename Batch>
void volume_feed_launch_as(const Batch& fb, int batch, const int32_t* origins, float* image_out, int64_t* label_out, int R0, int R1, int R2,
                           void* stream) {
  const long voxels = (long)R0 * R1 * R2;
  if constexpr (std::is_same_v<Batch, icl::VolumeFeedBatch>) {
    const dim3 grid(grid_for(voxels / V, 256, 8192), batch);      // one grid row per sample
    ICL_LAUNCH((icl::volume_feed_kernel<V, DEV>), grid, dim3(256), 0, (hipStream_t)stream, fb, (const int*)origins, image_out,
               (long long*)label_out, R0, R1, R2);
  } else {
    // an affine sample takes one thread per output voxel whatever V, as for icl_crop_rotflip_affine; with none, volume_feed_kernel's grid
    bool any = false;
    for (int b = 0; b < batch; ++b) any = any || fb.s[b].affine;
    const dim3 grid(grid_for(any ? voxels : voxels / V, 256, 8192), batch);
    ICL_LAUNCH((icl::volume_feed_affine_kernel<V, DEV>), grid, dim3(256), 0, (hipStream_t)stream, fb, (const int*)origins, image_out,
               (long long*)label_out, R0, R1, R2);
  }
}

// The launch of a filled batch, VolumeFeedBatch through volume_feed_kernel and VolumeFeedAffineBatch through volume_feed_affine_kernel:
// a quad per thread where the depth and both outputs allow 16-byte stores; origins: the device origins, or nullptr for the records' own.
extern "C++" template <typename Batch>
int volume_feed_launch(const char* what, const Batch& fb, int batch, const int32_t* origins, float* image_out, int64_t* label_out, int R0,
                       int R1, int R2, void* stream) {
  const bool quad = (R2 & 3) == 0 && aligned16(image_out) && aligned16(label_out);
  if (quad && origins) volume_feed_launch_as<4, true>(fb, batch, origins, image_out, label_out, R0, R1, R2, stream);
  else if (quad) volume_feed_launch_as<4, false>(fb, batch, origins, image_out, label_out, R0, R1, R2, stream);
  else if (origins) volume_feed_launch_as<1, true>(fb, batch, origins, image_out, label_out, R0, R1, R2, stream);
  else volume_feed_launch_as<1, false>(fb, batch, origins, image_out, label_out, R0, R1, R2, stream);
  return check_launch(what);
}

// extents of a volume the rank index takes: MONAI casts crop centres to uint16, and the index counts in uint32
int rank_extents_ok(const char* what, int b, int n0, int n1, int n2) {
  if (n0 < 1 || n1 < 1 || n2 < 1 || n0 > 65535 || n1 > 65535 || n2 > 65535)
    return fail(-1, "%s: sample %d: extents %d x %d x %d (each must be in 1..65535)", what, b, n0, n1, n2);
  if ((long)n0 * n1 * n2 > 0x7fffffffL) return fail(-1, "%s: sample %d: extents %d x %d x %d (more than 2^31 - 1 voxels)", what, b, n0, n1, n2);
  return 0;
}

inline bool rank_vec_ok(const void* image, const void* label) { return aligned16(image) && ((uintptr_t)label & 3) == 0; }

}  // namespace

int icl_volume_feed(const void* const* images, const void* const* labels, const int32_t* int_params, const float* float_params, int batch,
                    float* image_out, int64_t* label_out, int R0, int R1, int R2, void* stream) {
  if (!images || !labels || !int_params || !float_params || !image_out || !label_out) return fail(-1, "volume_feed: null pointer");
  icl::VolumeFeedBatch fb{};
  if (const int rc = volume_feed_records("volume_feed", images, labels, int_params, float_params, batch, R0, R1, R2, false, fb)) return rc;
  return volume_feed_launch("volume_feed", fb, batch, nullptr, image_out, label_out, R0, R1, R2, stream);
}

int icl_volume_feed_origins(const void* const* images, const void* const* labels, const int32_t* int_params, const float* float_params,
                            int batch, const int32_t* origins, float* image_out, int64_t* label_out, int R0, int R1, int R2, void* stream) {
  if (!images || !labels || !int_params || !float_params || !origins || !image_out || !label_out)
    return fail(-1, "volume_feed_origins: null pointer");
  icl::VolumeFeedBatch fb{};
  if (const int rc = volume_feed_records("volume_feed_origins", images, labels, int_params, float_params, batch, R0, R1, R2, true, fb))
    return rc;
  return volume_feed_launch("volume_feed_origins", fb, batch, origins, image_out, label_out, R0, R1, R2, stream);
}

namespace {

// The records of icl_volume_feed_affine / icl_volume_feed_affine_origins: volume_feed_records' rows and checks, then the affine rows.
int volume_feed_affine_records(const char* what, const void* const* images, const void* const* labels, const int32_t* int_params,
                               const float* float_params, const double* affine_params, int batch, int R0, int R1, int R2, bool device_origins,
                               icl::VolumeFeedAffineBatch& ab) {
  static_assert(sizeof(icl::VolumeFeedAffineBatch) == 16 * 160, "16 records of 160 B: 2,560 B of the 4 KB kernel-argument block");
  if (!affine_params) return fail(-1, "%s: affine_params is a null pointer", what);
  icl::VolumeFeedBatch fb{};
  if (const int rc = volume_feed_records(what, images, labels, int_params, float_params, batch, R0, R1, R2, device_origins, fb)) return rc;
  for (int b = 0; b < batch; ++b) {
    ab.s[b].f = fb.s[b];
    ab.s[b].n0 = int_params[14 * b];
    if (const int rc = affine_rows(what, affine_params, b, ab.s[b].affine, ab.s[b].m)) return rc;
  }
  return 0;
}

}  // namespace

int icl_volume_feed_affine(const void* const* images, const void* const* labels, const int32_t* int_params, const float* float_params,
                           const double* affine_params, int batch, float* image_out, int64_t* label_out, int R0, int R1, int R2, void* stream) {
  if (!images || !labels || !int_params || !float_params || !image_out || !label_out) return fail(-1, "volume_feed_affine: null pointer");
  icl::VolumeFeedAffineBatch ab{};
  if (const int rc = volume_feed_affine_records("volume_feed_affine", images, labels, int_params, float_params, affine_params, batch, R0, R1,
                                                R2, false, ab))
    return rc;
  return volume_feed_launch("volume_feed_affine", ab, batch, nullptr, image_out, label_out, R0, R1, R2, stream);
}

int icl_volume_feed_affine_origins(const void* const* images, const void* const* labels, const int32_t* int_params, const float* float_params,
                                   const double* affine_params, int batch, const int32_t* origins, float* image_out, int64_t* label_out,
                                   int R0, int R1, int R2, void* stream) {
  if (!images || !labels || !int_params || !float_params || !origins || !image_out || !label_out)
    return fail(-1, "volume_feed_affine_origins: null pointer");
  icl::VolumeFeedAffineBatch ab{};
  if (const int rc = volume_feed_affine_records("volume_feed_affine_origins", images, labels, int_params, float_params, affine_params, batch,
                                                R0, R1, R2, true, ab))
    return rc;
  return volume_feed_launch("volume_feed_affine_origins", ab, batch, origins, image_out, label_out, R0, R1, R2, stream);
}

int icl_rank_tile(void) { return icl::kRankTile; }

int icl_rank_index_build(const float* image, const uint8_t* label, int n0, int n1, int n2, float threshold, uint32_t* fg_index,
                         uint32_t* bg_index, void* stream) {
  if (!image || !label || !fg_index || !bg_index) return fail(-1, "rank_index_build: null pointer");
  if (const int rc = rank_extents_ok("rank_index_build", 0, n0, n1, n2)) return rc;
  const long total = (long)n0 * n1 * n2;
  const int tiles = (int)cdivl(total, icl::kRankTile);
  ICL_LAUNCH(icl::rank_count_kernel, dim3(tiles), dim3(icl::kRankThreads), 0, (hipStream_t)stream, image, label, (unsigned*)fg_index,
             (unsigned*)bg_index, total, threshold, rank_vec_ok(image, label) ? 1 : 0);
  if (const int rc = check_launch("rank_count")) return rc;
  ICL_LAUNCH(icl::rank_scan_kernel, dim3(2), dim3(icl::kRankThreads), 0, (hipStream_t)stream, (unsigned*)fg_index, (unsigned*)bg_index, tiles);
  return check_launch("rank_scan");
}

int icl_rank_select(const void* const* images, const void* const* labels, const void* const* fg_indices, const void* const* bg_indices,
                    const int32_t* int_params, float threshold, int batch, int32_t* origins, void* stream) {
  if (!images || !labels || !fg_indices || !bg_indices || !int_params || !origins) return fail(-1, "rank_select: null pointer");
  if (batch < 1 || batch > icl::kFeedMaxBatch) return fail(-1, "rank_select: batch %d out of range (1 <= batch <= %d)", batch, icl::kFeedMaxBatch);
  icl::RankSelectBatch sb{};
  for (int b = 0; b < batch; ++b) {
    const int32_t* q = int_params + 8 * b;       // n[3], kind, rank, s[3]
    icl::RankSelectSample& s = sb.s[b];
    s.image = (const float*)images[b];
    s.label = (const uint8_t*)labels[b];
    if (!s.image || !s.label || !fg_indices[b] || !bg_indices[b]) return fail(-1, "rank_select: sample %d: null volume or index pointer", b);
    if (const int rc = rank_extents_ok("rank_select", b, q[0], q[1], q[2])) return rc;
    s.n0 = q[0]; s.n1 = q[1]; s.n2 = q[2];
    s.kind = q[3]; s.rank = q[4];
    s.s0 = q[5]; s.s1 = q[6]; s.s2 = q[7];
    if (s.kind != icl::kRankFg && s.kind != icl::kRankBg) return fail(-1, "rank_select: sample %d: kind %d (0 foreground, 1 background)", b, s.kind);
    if (s.rank < 0) return fail(-1, "rank_select: sample %d: rank %d (must be >= 0)", b, s.rank);
    for (int a = 0; a < 3; ++a)
      if (q[5 + a] < 1 || q[5 + a] > q[a]) return fail(-1, "rank_select: sample %d: crop size %d of axis %d outside 1..%d", b, q[5 + a], a, q[a]);
    s.prefix = (const unsigned*)(s.kind == icl::kRankFg ? fg_indices[b] : bg_indices[b]);
    s.tiles = (int)cdivl((long)s.n0 * s.n1 * s.n2, icl::kRankTile);
    s.vec = rank_vec_ok(s.image, s.label) ? 1 : 0;
  }
  ICL_LAUNCH(icl::rank_select_kernel, dim3(batch), dim3(icl::kRankThreads), 0, (hipStream_t)stream, sb, threshold, (int*)origins);
  return check_launch("rank_select");
}

namespace {

// A prefix plan as the caller hands it over, checked once for icl_prefix_resample and icl_prefix_restore.  int_params [24] = {raw
// extents n[3], box lo[3], box hi[3] (exclusive), perm[3], sign[3], pad front f[3], padded extents m[3], output extents o[3]};
// double_params [6] = {source spacing s[3], target spacing p[3]}, both per ORIENTED axis.
struct PrefixPlanArgs {
  int n[3], lo[3], hi[3], perm[3], sign[3], f[3], m[3], o[3], e[3];
  double s[3], p[3];
};

int prefix_plan_args(const char* what, const int32_t* q, const double* d, PrefixPlanArgs& a) {
  for (int k = 0; k < 3; ++k) {
    a.n[k] = q[k]; a.lo[k] = q[3 + k]; a.hi[k] = q[6 + k]; a.perm[k] = q[9 + k]; a.sign[k] = q[12 + k];
    a.f[k] = q[15 + k]; a.m[k] = q[18 + k]; a.o[k] = q[21 + k];
    a.s[k] = d[k]; a.p[k] = d[3 + k];
  }
  if (a.n[0] < 1 || a.n[1] < 1 || a.n[2] < 1 || a.n[0] > 65535 || a.n[1] > 65535 || a.n[2] > 65535)
    return fail(-1, "%s: raw extents %d x %d x %d (each must be in 1..65535)", what, a.n[0], a.n[1], a.n[2]);
  if ((long)a.n[0] * a.n[1] * a.n[2] > 0x7fffffffL)
    return fail(-1, "%s: raw extents %d x %d x %d (more than 2^31 - 1 voxels)", what, a.n[0], a.n[1], a.n[2]);
  int seen = 0;
  for (int k = 0; k < 3; ++k) {
    if (a.perm[k] < 0 || a.perm[k] > 2) return fail(-1, "%s: perm (%d, %d, %d) is not a permutation of 0, 1, 2", what, a.perm[0], a.perm[1], a.perm[2]);
    seen |= 1 << a.perm[k];
    if (a.sign[k] != 1 && a.sign[k] != -1) return fail(-1, "%s: sign %d of oriented axis %d (1 or -1)", what, a.sign[k], k);
  }
  if (seen != 7) return fail(-1, "%s: perm (%d, %d, %d) is not a permutation of 0, 1, 2", what, a.perm[0], a.perm[1], a.perm[2]);
  for (int k = 0; k < 3; ++k)
    if (a.lo[k] < 0 || a.hi[k] <= a.lo[k] || a.hi[k] > a.n[k])
      return fail(-1, "%s: box [%d, %d) of raw axis %d outside the extent %d", what, a.lo[k], a.hi[k], k, a.n[k]);
  for (int k = 0; k < 3; ++k) {
    if (!std::isfinite(a.s[k]) || !std::isfinite(a.p[k]) || !(a.s[k] > 0.0) || !(a.p[k] > 0.0) || !std::isfinite(a.p[k] / a.s[k]) ||
        !(a.s[k] / a.p[k] > 0.0))
      return fail(-1, "%s: spacing %g -> %g of oriented axis %d (both must be finite and positive)", what, a.s[k], a.p[k], k);
    a.e[k] = a.hi[a.perm[k]] - a.lo[a.perm[k]];
    if (a.f[k] < 0 || a.m[k] > 65535 || (long)a.f[k] + a.e[k] > a.m[k])
      return fail(-1, "%s: pad front %d + crop extent %d of oriented axis %d outside the padded extent %d (at most 65535)", what, a.f[k],
                  a.e[k], k, a.m[k]);
    const double want = std::nearbyint((double)(a.m[k] - 1) * (a.s[k] / a.p[k]) + 1.0);      // round half to even
    if (!(want >= 1.0 && want <= 65535.0) || a.o[k] != (int)want)
      return fail(-1, "%s: output extent %d of oriented axis %d: rint((%d - 1) * (%g / %g) + 1) = %.0f (must be in 1..65535)", what, a.o[k], k,
                  a.m[k], a.s[k], a.p[k], want);
  }
  if ((long)a.o[0] * a.o[1] * a.o[2] > 0x7fffffffL)
    return fail(-1, "%s: output extents %d x %d x %d (more than 2^31 - 1 voxels)", what, a.o[0], a.o[1], a.o[2]);
  return 0;
}

int prefix_window_args(const char* what, const float* window, int clip, icl::PrefixWindow& w) {
  w.a_min = window[0]; w.a_range = window[1]; w.b_min = window[2]; w.b_range = window[3]; w.b_max = window[4];
  w.clip = clip ? 1 : 0;
  for (int i = 0; i < 5; ++i)
    if (!std::isfinite(window[i])) return fail(-1, "%s: window constant %d is not finite", what, i);
  if (w.a_range == 0.f) return fail(-1, "%s: a_max - a_min is 0", what);
  return 0;
}

}  // namespace

int icl_prefix_box(const float* image, int n0, int n1, int n2, const float* window, int clip, int32_t* box, int32_t* ws, void* stream) {
  if (!image || !window || !box || !ws) return fail(-1, "prefix_box: null pointer");
  if (n0 < 1 || n1 < 1 || n2 < 1 || n0 > 65535 || n1 > 65535 || n2 > 65535)
    return fail(-1, "prefix_box: extents %d x %d x %d (each must be in 1..65535)", n0, n1, n2);
  if ((long)n0 * n1 * n2 > 0x7fffffffL) return fail(-1, "prefix_box: extents %d x %d x %d (more than 2^31 - 1 voxels)", n0, n1, n2);
  icl::PrefixWindow w;
  if (const int rc = prefix_window_args("prefix_box", window, clip, w)) return rc;
  const long total = (long)n0 * n1 * n2;
  const int blocks = grid_for(cdivl(total, 4), icl::kPrefixThreads, icl::kPrefixBoxBlocks);
  ICL_LAUNCH(icl::prefix_box_partial_kernel, dim3(blocks), dim3(icl::kPrefixThreads), 0, (hipStream_t)stream, image, n1, n2, total, w,
             aligned16(image) ? 1 : 0, (int*)ws);
  if (const int rc = check_launch("prefix_box_partial")) return rc;
  ICL_LAUNCH(icl::prefix_box_finish_kernel, dim3(1), dim3(icl::kPrefixThreads), 0, (hipStream_t)stream, (const int*)ws, blocks, (int*)box);
  return check_launch("prefix_box_finish");
}

int icl_prefix_resample(const float* image, const uint8_t* label, const int32_t* int_params, const double* double_params, const float* window,
                        int clip, float* image_out, uint8_t* label_out, void* stream) {
  if (!image || !label || !int_params || !double_params || !window || !image_out || !label_out) return fail(-1, "prefix_resample: null pointer");
  PrefixPlanArgs a;
  if (const int rc = prefix_plan_args("prefix_resample", int_params, double_params, a)) return rc;
  icl::PrefixWindow w;
  if (const int rc = prefix_window_args("prefix_resample", window, clip, w)) return rc;
  icl::PrefixGeom g{};
  const long raw_stride[3] = {(long)a.n[1] * a.n[2], (long)a.n[2], 1L};
  for (int k = 0; k < 3; ++k) {
    const int r = a.perm[k];
    g.step[k] = a.sign[k] > 0 ? raw_stride[r] : -raw_stride[r];
    g.base += (long)(a.sign[k] > 0 ? a.lo[r] : a.hi[r] - 1) * raw_stride[r];
    g.e[k] = a.e[k]; g.f[k] = a.f[k]; g.m[k] = a.m[k]; g.o[k] = a.o[k];
    g.fwd[k] = a.p[k] / a.s[k];
  }
  // axis-2 outputs per tile: the taps of `tile2` consecutive outputs span at most floor((tile2 - 1) * fwd) + 3 slots (the two ends'
  // floors differ by at most floor(distance) + 1, and i1 adds one); one slot of margin is kept
  const double room = (double)(icl::kPrefixSlots - 4) / g.fwd[2];
  int tile2 = room >= (double)(icl::kPrefixTile2 - 1) ? icl::kPrefixTile2 : (int)room + 1;
  if (tile2 > a.o[2]) tile2 = a.o[2];
  const bool quads = (a.o[2] & 3) == 0 && aligned16(image_out) && ((uintptr_t)label_out & 3) == 0 && tile2 >= 4;
  if (quads) tile2 &= ~3;
  const long tiles = (long)a.o[0] * cdivl(a.o[1], icl::kPrefixRows) * cdivl(a.o[2], tile2);
  const dim3 grid(grid_for(tiles, 1, 65536));
  if (quads) {
    ICL_LAUNCH(icl::prefix_resample_kernel<4>, grid, dim3(icl::kPrefixThreads), 0, (hipStream_t)stream, image, label, g, w, tile2, image_out,
               label_out);
  } else {
    ICL_LAUNCH(icl::prefix_resample_kernel<1>, grid, dim3(icl::kPrefixThreads), 0, (hipStream_t)stream, image, label, g, w, tile2, image_out,
               label_out);
  }
  return check_launch("prefix_resample");
}

int icl_prefix_restore(const void* prediction, int elem_kind, const int32_t* int_params, const double* double_params, uint8_t* out,
                       void* stream) {
  if (!prediction || !int_params || !double_params || !out) return fail(-1, "prefix_restore: null pointer");
  if (elem_kind != 0 && elem_kind != 1) return fail(-1, "prefix_restore: unknown element kind %d (0 uint8, 1 int64)", elem_kind);
  PrefixPlanArgs a;
  if (const int rc = prefix_plan_args("prefix_restore", int_params, double_params, a)) return rc;
  icl::PrefixRestoreGeom g{};
  const long pred_stride[3] = {(long)a.o[1] * a.o[2], (long)a.o[2], 1L};
  for (int k = 0; k < 3; ++k) {          // oriented axis k is raw axis r
    const int r = a.perm[k];
    g.n[r] = a.n[r]; g.lo[r] = a.lo[r]; g.hi[r] = a.hi[r];
    g.rev[r] = a.sign[k] < 0 ? 1 : 0;
    g.f[r] = a.f[k]; g.o[r] = a.o[k];
    g.pstride[r] = pred_stride[k];
    g.inv[r] = a.s[k] / a.p[k];
  }
  const long voxels = (long)a.n[0] * a.n[1] * a.n[2];
  const dim3 grid(grid_for(voxels, icl::kPrefixThreads, 8192));
  if (elem_kind == 0) {
    ICL_LAUNCH(icl::prefix_restore_kernel<uint8_t>, grid, dim3(icl::kPrefixThreads), 0, (hipStream_t)stream, (const uint8_t*)prediction, g, out);
  } else {
    ICL_LAUNCH(icl::prefix_restore_kernel<long long>, grid, dim3(icl::kPrefixThreads), 0, (hipStream_t)stream, (const long long*)prediction, g,
               out);
  }
  return check_launch("prefix_restore");
}

namespace {

// what the intensity entry points share: the batch pointer, the batch size and the patch extents
int intensity_common(const char* what, const void* image, int batch, int R0, int R1, int R2) {
  if (!image) return fail(-1, "%s: null pointer", what);
  if (batch < 1 || batch > icl::kFeedMaxBatch) return fail(-1, "%s: batch %d out of range (1 <= batch <= %d)", what, batch, icl::kFeedMaxBatch);
  if (R0 < 1 || R1 < 1 || R2 < 1) return fail(-1, "%s: extents %d x %d x %d (each must be >= 1)", what, R0, R1, R2);
  if ((long)R0 * R1 * R2 > 0x7fffffffL) return fail(-1, "%s: extents %d x %d x %d (more than 2^31 - 1 voxels a sample)", what, R0, R1, R2);
  return 0;
}

// a flag travels as a double beside the other values of its row: exactly 0 or 1
int intensity_flag(const char* what, int b, const char* name, double v, int& out) {
  if (!(v == 0.0 || v == 1.0)) return fail(-1, "%s: sample %d: %s flag %g (must be 0 or 1)", what, b, name, v);
  out = v == 1.0 ? 1 : 0;
  return 0;
}

}  // namespace

int icl_intensity_noise(float* image, const double* params, int batch, int R0, int R1, int R2, void* stream) {
  if (!params) return fail(-1, "intensity_noise: null pointer");
  if (const int rc = intensity_common("intensity_noise", image, batch, R0, R1, R2)) return rc;
  icl::NoiseBatch nb{};
  bool any = false;
  for (int b = 0; b < batch; ++b) {
    const double* q = params + 4 * b;      // flag, seed, sigma, clip
    icl::NoiseSample& s = nb.s[b];
    if (const int rc = intensity_flag("intensity_noise", b, "noise", q[0], s.on)) return rc;
    if (!(q[1] >= 0.0 && q[1] <= 4294967295.0) || q[1] != std::floor(q[1]))
      return fail(-1, "intensity_noise: sample %d: seed %g (must be an integer in 0 .. 2^32 - 1)", b, q[1]);
    if (!std::isfinite(q[2]) || !(q[2] > 0.0)) return fail(-1, "intensity_noise: sample %d: sigma %g (must be finite and positive)", b, q[2]);
    if (!std::isfinite(q[3]) || q[3] < 0.0) return fail(-1, "intensity_noise: sample %d: clip %g (must be finite; 0 means none)", b, q[3]);
    s.seed = (unsigned)q[1];
    s.sigma = q[2];
    s.clip = q[3] > 0.0 ? 1 : 0;
    s.limit = (float)(q[3] * q[2]);
    any = any || s.on;
  }
  if (!any) return 0;
  const long voxels = (long)R0 * R1 * R2;
  if ((R2 & 3) == 0 && aligned16(image)) {
    ICL_LAUNCH((icl::intensity_noise_kernel<4>), dim3(grid_for(voxels / 4, icl::kIntensityThreads, 8192), batch), dim3(icl::kIntensityThreads), 0,
               (hipStream_t)stream, nb, image, (unsigned)voxels);
  } else {
    ICL_LAUNCH((icl::intensity_noise_kernel<1>), dim3(grid_for(voxels, icl::kIntensityThreads, 8192), batch), dim3(icl::kIntensityThreads), 0,
               (hipStream_t)stream, nb, image, (unsigned)voxels);
  }
  return check_launch("intensity_noise");
}

int icl_intensity_blur(float* image, float* scratch, const double* params, int batch, int R0, int R1, int R2, void* stream) {
  if (!scratch || !params) return fail(-1, "intensity_blur: null pointer");
  if (const int rc = intensity_common("intensity_blur", image, batch, R0, R1, R2)) return rc;
  if (image == scratch) return fail(-1, "intensity_blur: the scratch buffer is the batch itself");
  if (R2 > icl::kBlurLineFloats) return fail(-1, "intensity_blur: extent %d of the contiguous axis (at most %d)", R2, icl::kBlurLineFloats);
  const int smallest = R0 < R1 ? (R0 < R2 ? R0 : R2) : (R1 < R2 ? R1 : R2);
  icl::BlurBatch bb{};
  bool any = false;
  for (int b = 0; b < batch; ++b) {
    const double* q = params + (2 + icl::kBlurMaxRadius + 1) * b;      // flag, sigma, w_0 .. w_12
    icl::BlurSample& s = bb.s[b];
    int flag = 0;
    if (const int rc = intensity_flag("intensity_blur", b, "blur", q[0], flag)) return rc;
    if (!std::isfinite(q[1]) || !(q[1] > 0.0)) return fail(-1, "intensity_blur: sample %d: sigma %g (must be finite and positive)", b, q[1]);
    const double rr = std::floor(4.0 * q[1] + 0.5);                   // int(4 sigma + 0.5), on the double
    if (rr > (double)icl::kBlurMaxRadius)
      return fail(-1, "intensity_blur: sample %d: sigma %g gives the radius %.0f (at most %d)", b, q[1], rr, icl::kBlurMaxRadius);
    s.r = (int)rr;
    if (s.r > smallest)
      return fail(-1, "intensity_blur: sample %d: radius %d above the smallest extent of %d x %d x %d", b, s.r, R0, R1, R2);
    for (int k = 0; k <= s.r; ++k) {
      if (!(q[2 + k] >= 0.0 && q[2 + k] <= 1.0)) return fail(-1, "intensity_blur: sample %d: weight w[%d] = %g outside [0, 1]", b, k, q[2 + k]);
      s.w[k] = q[2 + k];
    }
    s.on = flag && s.r > 0 ? 1 : 0;                                   // r = 0: w_0 = 1, the identity
    any = any || s.on;
  }
  if (!any) return 0;
  const long voxels = (long)R0 * R1 * R2;
  const dim3 block(icl::kIntensityThreads);
  {   // axis 0: batch -> scratch
    const long tiles = cdivl(R0, icl::kBlurTileL) * cdivl((long)R1 * R2, icl::kBlurTileI);
    ICL_LAUNCH(icl::intensity_blur_strided_kernel, dim3(grid_for(tiles, 1, 8192), batch), block, 0, (hipStream_t)stream, bb, (const float*)image,
               scratch, 1, R0, R1 * R2, (unsigned)voxels);
    if (const int rc = check_launch("intensity_blur axis 0")) return rc;
  }
  {   // axis 1: scratch -> batch
    const long tiles = (long)R0 * cdivl(R1, icl::kBlurTileL) * cdivl(R2, icl::kBlurTileI);
    ICL_LAUNCH(icl::intensity_blur_strided_kernel, dim3(grid_for(tiles, 1, 8192), batch), block, 0, (hipStream_t)stream, bb, (const float*)scratch,
               image, R0, R1, R2, (unsigned)voxels);
    if (const int rc = check_launch("intensity_blur axis 1")) return rc;
  }
  const int lines = R0 * R1;                                          // axis 2: in place, whole lines through LDS
  const int lpb = icl::kBlurLineFloats / R2;
  const dim3 grid(grid_for(cdivl(lines, lpb), 1, 8192), batch);
  if ((R2 & 3) == 0 && aligned16(image)) {
    ICL_LAUNCH((icl::intensity_blur_line_kernel<4>), grid, block, 0, (hipStream_t)stream, bb, image, lines, R2, lpb, (unsigned)voxels);
  } else {
    ICL_LAUNCH((icl::intensity_blur_line_kernel<1>), grid, block, 0, (hipStream_t)stream, bb, image, lines, R2, lpb, (unsigned)voxels);
  }
  return check_launch("intensity_blur axis 2");
}

int icl_intensity_lowres(float* image, float* scratch, const int32_t* params, int batch, int R0, int R1, int R2, void* stream) {
  if (!scratch || !params) return fail(-1, "intensity_lowres: null pointer");
  if (const int rc = intensity_common("intensity_lowres", image, batch, R0, R1, R2)) return rc;
  if (image == scratch) return fail(-1, "intensity_lowres: the scratch buffer is the batch itself");
  const int R[3] = {R0, R1, R2};
  icl::LowresBatch lb{};
  bool any = false;
  for (int b = 0; b < batch; ++b) {
    const int32_t* q = params + 4 * b;     // flag, L0, L1, L2
    icl::LowresSample& s = lb.s[b];
    if (q[0] != 0 && q[0] != 1) return fail(-1, "intensity_lowres: sample %d: flag %d (must be 0 or 1)", b, q[0]);
    bool smaller = false;
    for (int a = 0; a < 3; ++a) {
      if (q[1 + a] < 1 || q[1 + a] > R[a])
        return fail(-1, "intensity_lowres: sample %d: low extent %d of axis %d (must be in 1 .. %d)", b, q[1 + a], a, R[a]);
      s.L[a] = q[1 + a];
      s.sn[a] = (float)R[a] / (float)q[1 + a];
      s.sl[a] = (float)q[1 + a] / (float)R[a];
      smaller = smaller || q[1 + a] < R[a];
    }
    s.on = q[0] == 1 && smaller ? 1 : 0;                              // every L = R: the identity
    any = any || s.on;
  }
  if (!any) return 0;
  const long voxels = (long)R0 * R1 * R2;
  const dim3 block(icl::kIntensityThreads);
  if ((R2 & 3) == 0 && aligned16(image) && aligned16(scratch)) {
    const dim3 grid(grid_for(voxels / 4, icl::kIntensityThreads, 8192), batch);
    ICL_LAUNCH((icl::intensity_lowres_kernel<4>), grid, block, 0, (hipStream_t)stream, lb, (const float*)image, scratch, R0, R1, R2,
               (unsigned)voxels);
    if (const int rc = check_launch("intensity_lowres gather")) return rc;
    ICL_LAUNCH((icl::intensity_lowres_copy_kernel<4>), grid, block, 0, (hipStream_t)stream, lb, (const float*)scratch, image, (unsigned)voxels);
  } else {
    const dim3 grid(grid_for(voxels, icl::kIntensityThreads, 8192), batch);
    ICL_LAUNCH((icl::intensity_lowres_kernel<1>), grid, block, 0, (hipStream_t)stream, lb, (const float*)image, scratch, R0, R1, R2,
               (unsigned)voxels);
    if (const int rc = check_launch("intensity_lowres gather")) return rc;
    ICL_LAUNCH((icl::intensity_lowres_copy_kernel<1>), grid, block, 0, (hipStream_t)stream, lb, (const float*)scratch, image, (unsigned)voxels);
  }
  return check_launch("intensity_lowres copy");
}

int icl_intensity_stats(const float* image, const int32_t* flags, int batch, int R0, int R1, int R2, float* stats, double* ws, void* stream) {
  if (!flags || !stats || !ws) return fail(-1, "intensity_stats: null pointer");
  if (const int rc = intensity_common("intensity_stats", image, batch, R0, R1, R2)) return rc;
  icl::IntensityFlags fl{};
  bool any = false;
  for (int b = 0; b < batch; ++b) {
    if (flags[b] != 0 && flags[b] != 1) return fail(-1, "intensity_stats: sample %d: flag %d (must be 0 or 1)", b, flags[b]);
    fl.on[b] = flags[b];
    any = any || fl.on[b];
  }
  if (!any) return 0;
  const long voxels = (long)R0 * R1 * R2;
  const int blocks = grid_for(cdivl(voxels, 4), icl::kIntensityThreads, icl::kIntensityStatBlocks);
  ICL_LAUNCH(icl::intensity_stats_partial_kernel, dim3(blocks, batch), dim3(icl::kIntensityThreads), 0, (hipStream_t)stream, fl, image,
             (unsigned)voxels, (voxels & 3) == 0 && aligned16(image) ? 1 : 0, ws);
  if (const int rc = check_launch("intensity_stats_partial")) return rc;
  ICL_LAUNCH(icl::intensity_stats_finish_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, fl, (const double*)ws, batch, blocks,
             (unsigned)voxels, stats);
  return check_launch("intensity_stats_finish");
}

int icl_intensity_point(float* image, const float* stats, const double* params, int batch, int R0, int R1, int R2, void* stream) {
  if (!stats || !params) return fail(-1, "intensity_point: null pointer");
  if (const int rc = intensity_common("intensity_point", image, batch, R0, R1, R2)) return rc;
  icl::PointBatch pb{};
  bool any = false;
  for (int b = 0; b < batch; ++b) {
    const double* q = params + 5 * b;      // contrast flag, f, gamma flag, g, invert flag
    icl::PointSample& s = pb.s[b];
    if (const int rc = intensity_flag("intensity_point", b, "contrast", q[0], s.contrast)) return rc;
    if (const int rc = intensity_flag("intensity_point", b, "gamma", q[2], s.gamma)) return rc;
    if (const int rc = intensity_flag("intensity_point", b, "invert", q[4], s.invert)) return rc;
    s.f = (float)q[1];
    if (!std::isfinite(q[1]) || !std::isfinite(s.f) || !(s.f > 0.f))
      return fail(-1, "intensity_point: sample %d: contrast factor %g (must be finite and positive in fp32)", b, q[1]);
    if (!std::isfinite(q[3]) || !(q[3] > 0.0)) return fail(-1, "intensity_point: sample %d: gamma %g (must be finite and positive)", b, q[3]);
    s.g = q[3];
    if (!s.gamma) s.invert = 0;
    any = any || s.contrast || s.gamma;
  }
  if (!any) return 0;
  const long voxels = (long)R0 * R1 * R2;
  if ((R2 & 3) == 0 && aligned16(image)) {
    ICL_LAUNCH((icl::intensity_point_kernel<4>), dim3(grid_for(voxels / 4, icl::kIntensityThreads, 8192), batch), dim3(icl::kIntensityThreads), 0,
               (hipStream_t)stream, pb, stats, image, (unsigned)voxels);
  } else {
    ICL_LAUNCH((icl::intensity_point_kernel<1>), dim3(grid_for(voxels, icl::kIntensityThreads, 8192), batch), dim3(icl::kIntensityThreads), 0,
               (hipStream_t)stream, pb, stats, image, (unsigned)voxels);
  }
  return check_launch("intensity_point");
}

int icl_slice_augment(const void* const* images, const void* const* labels, const int32_t* int_params, const double* double_params,
                      int batch, float* image_out, uint8_t* label_out, int o0, int o1, void* stream) {
  if (!images || !labels || !int_params || !double_params || !image_out || !label_out)
    return fail(-1, "slice_augment: null pointer");
  if (batch < 1 || batch > icl::kSliceMaxBatch) return fail(-1, "slice_augment: batch %d out of range (1 <= batch <= %d)", batch, icl::kSliceMaxBatch);
  if (o0 < 2 || o1 < 2) return fail(-1, "slice_augment: output extents %d x %d (each must be >= 2)", o0, o1);
  if ((long)o0 * o1 > 0x7fffffffL) return fail(-1, "slice_augment: output extents %d x %d (more than 2^31 - 1 pixels a sample)", o0, o1);
  icl::SliceBatch sb{};
  for (int b = 0; b < batch; ++b) {
    const int32_t* q = int_params + 5 * b;
    const double* d = double_params + 8 * b;
    icl::SliceSample& s = sb.s[b];
    s.image = (const float*)images[b];
    s.label = (const uint8_t*)labels[b];
    s.n0 = q[0]; s.n1 = q[1]; s.branch = q[2]; s.k = q[3]; s.flip_axis = q[4];
    s.m00 = d[0]; s.m01 = d[1]; s.m10 = d[2]; s.m11 = d[3]; s.off0 = d[4]; s.off1 = d[5]; s.z0 = d[6]; s.z1 = d[7];
    if (!s.image || !s.label) return fail(-1, "slice_augment: sample %d: null slice pointer", b);
    if (s.n0 < 1 || s.n1 < 1) return fail(-1, "slice_augment: sample %d: extents %d x %d (each must be >= 1)", b, s.n0, s.n1);
    if (s.branch < icl::kSliceNone || s.branch > icl::kSliceRotate) return fail(-1, "slice_augment: sample %d: unknown branch %d", b, s.branch);
    if (s.branch == icl::kSliceRotFlip && (s.k < 0 || s.k > 3)) return fail(-1, "slice_augment: sample %d: k = %d outside 0..3", b, s.k);
    if (s.branch == icl::kSliceRotFlip && (s.flip_axis < 0 || s.flip_axis > 1))
      return fail(-1, "slice_augment: sample %d: flip axis %d (0 or 1)", b, s.flip_axis);
  }
  ICL_LAUNCH(icl::slice_augment_kernel, dim3(grid_for((long)batch * o0 * o1, 256, 8192)), dim3(256), 0, (hipStream_t)stream, sb, image_out,
             label_out, batch, o0, o1);
  return check_launch("slice_augment");
}

int icl_slice_resize(const void* src, void* dst, int64_t batch, int n0, int n1, int o0, int o1, int elem_kind, void* stream) {
  if (!src || !dst) return fail(-1, "slice_resize: null pointer");
  if (batch < 1 || batch > (1 << 20)) return fail(-1, "slice_resize: batch %lld out of range", (long long)batch);
  if (n0 < 1 || n1 < 1) return fail(-1, "slice_resize: source extents %d x %d (each must be >= 1)", n0, n1);
  if (o0 < 2 || o1 < 2) return fail(-1, "slice_resize: output extents %d x %d (each must be >= 2)", o0, o1);
  if ((long)o0 * o1 > 0x7fffffffL) return fail(-1, "slice_resize: output extents %d x %d (more than 2^31 - 1 pixels a slice)", o0, o1);
  // scipy derives the factors from the extents: (n_in - 1) / (n_out - 1) in double
  const double z0 = (double)(n0 - 1) / (double)(o0 - 1), z1 = (double)(n1 - 1) / (double)(o1 - 1);
  const dim3 grid(grid_for((long)batch * o0 * o1, 256, 8192));
  if (elem_kind == 0) {
    ICL_LAUNCH(icl::slice_resize_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float*)src, (float*)dst, (int)batch, n0, n1, o0,
               o1, z0, z1);
  } else if (elem_kind == 1) {
    ICL_LAUNCH(icl::slice_resize_kernel<long long>, grid, dim3(256), 0, (hipStream_t)stream, (const long long*)src, (long long*)dst, (int)batch,
               n0, n1, o0, o1, z0, z1);
  } else {
    return fail(-1, "slice_resize: unknown element kind %d (0 fp32, 1 int64)", elem_kind);
  }
  return check_launch("slice_resize");
}

int icl_linear_dgrad_sgd(const float* gy, const float* x, float* w, float* mom, float* gx, void* ws, int64_t rows, int in, int out,
                         float lr, float momentum, float weight_decay, int first, const float* lr_dev, void* stream) {
  if (!gy || !x || !w || !mom || !gx || !ws || rows < 1 || rows > 32 || in < 4 || out < 4 || (in & 3) || (out & 3))
    return fail(-1, "linear_dgrad_sgd: bad argument (<= 32 rows, in / out multiples of 4, workspace of icl_linear_ws_bytes(.., 3))");
  if (!aligned16(gy) || !aligned16(x) || !aligned16(w) || !aligned16(mom) || !aligned16(gx)) return fail(-1, "linear_dgrad_sgd: 16-byte alignment");
  hipStream_t st = (hipStream_t)stream;
  const StreamPlan p = stream_plan((long)rows, in, out, true);
  const dim3 grid(p.groups, p.nslice);
  const size_t lds = ((size_t)16 * p.mt * p.slice_len + 8 * 1024) * 4;
  float* slab = (float*)ws;
  if (p.mt == 1) {
    ICL_SET_MAX_DYN_LDS((icl::linear_dgrad_sgd_kernel<1, 3>), 160 * 1024);
    ICL_LAUNCH((icl::linear_dgrad_sgd_kernel<1, 3>), grid, dim3(512), lds, st, gy, x, w, mom, slab, (int)rows, in, out, p.slice_len, p.upw, lr,
               momentum, weight_decay, first, lr_dev);
  } else {
    ICL_SET_MAX_DYN_LDS((icl::linear_dgrad_sgd_kernel<2, 2>), 160 * 1024);
    ICL_LAUNCH((icl::linear_dgrad_sgd_kernel<2, 2>), grid, dim3(512), lds, st, gy, x, w, mom, slab, (int)rows, in, out, p.slice_len, p.upw, lr,
               momentum, weight_decay, first, lr_dev);
  }
  if (int rc = check_launch("linear_dgrad_sgd")) return rc;
  ICL_LAUNCH(icl::gemm_reduce_slabs_kernel, dim3(grid_for(rows * (in / 4), 256, 1024)), dim3(256), 0, st, (const float*)slab, gx,
             (const float*)nullptr, p.nslice, (long)rows, in, (long)in, (long)16 * p.mt * in, (long)in, 0);
  return check_launch("linear_dgrad_sgd_reduce");
}

}  // extern "C"

#if defined(BF3_DEBUG) && (BF3_DEBUG & 16)
extern "C" int icl_debug_bf3_stamps(long long* dst) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(icl::g_bf3_stamps), sizeof(long long) * 2 * 3 * 32);
}
#endif

#if defined(WGTR_DEBUG)
extern "C" int icl_debug_wgtr_stamps(long long* dst) {
  return (int)hipMemcpyFromSymbol(dst, HIP_SYMBOL(icl::g_wgtr_stamps), sizeof(long long) * 2 * 4 * 8);
}
#endif

// ---------------------------------------------------------------- the aligner's query chain as fused stages (kernels/qchain.h)
int icl_qchain_stage(const IclQcStage* st, void* stream) {
  if (!st || !st->y || st->R < 1 || st->R > 32 || st->K < 1 || st->K > icl::kQcMaxK || st->nc < 1)
    return fail(-1, "qchain_stage: bad argument");
  static_assert(sizeof(IclQcStage) == sizeof(icl::QcStage), "IclQcStage and icl::QcStage must have the same layout");
  icl::QcStage s;
  memcpy(&s, st, sizeof(s));
  hipStream_t hs = (hipStream_t)stream;
  if ((s.pro == icl::QC_PRO_LN || s.pro == icl::QC_PRO_LNBWD) && !s.x) return fail(-1, "qchain_stage: the LayerNorm prologues need input rows");
  if (s.pro == icl::QC_PRO_LNBWD && (!s.pa || !s.pb)) return fail(-1, "qchain_stage: LayerNorm backward needs xhat and rstd");
  if ((s.epi == icl::QC_EPI_RES_DP || s.epi == icl::QC_EPI_GELUBWD) && !s.ea) return fail(-1, "qchain_stage: the epilogue needs its rows");
  if (s.trans == 2) {
    if (s.epi == icl::QC_EPI_SUMB && s.R > icl::kQcRB) return fail(-1, "qchain_stage: the batch sum needs all rows in one pass");
    s.N = s.K;
    ICL_LAUNCH(icl::qc_stage_rows_kernel, dim3(1), dim3(256), (size_t)icl::kQcRB * s.K * 4, hs, s);
    return check_launch("qc_stage_rows");
  }
  if (!s.w || s.N < 1) return fail(-1, "qchain_stage: bad product");
  if (s.trans == 0) {
    if (s.K % 4) return fail(-1, "qchain_stage: K must be a multiple of 4");
    s.npw = s.N >= 1024 ? 4 : s.N >= 256 ? 2 : 1;
    const int per_wg = 4 * s.npw;
    ICL_LAUNCH(icl::qc_stage_fwd_kernel, dim3((s.N + per_wg - 1) / per_wg), dim3(256), (size_t)icl::kQcRB * s.K * 4, hs, s);
    return check_launch("qc_stage_fwd");
  }
  if (s.trans != 1 || s.N % 4) return fail(-1, "qchain_stage: trans must be 0, 1 or 2 and N a multiple of 4");
  const size_t lds = ((size_t)icl::kQcRB * icl::kQcMaxK + icl::kQcBwdWaves * icl::kQcRB * 64) * 4;      // 48 KB
  ICL_LAUNCH(icl::qc_stage_bwd_kernel, dim3((s.N + 63) / 64), dim3(64 * icl::kQcBwdWaves), lds, hs, s);
  return check_launch("qc_stage_bwd");
}

int icl_qchain_wgrad(const void* const* g, const void* const* x, void* const* dw, void* const* db, const int32_t* rows, const int32_t* n,
                     const int32_t* k, const int32_t* kind, int count, void* stream) {
  if (!g || !x || !dw || !rows || !n || !k || !kind || count < 1 || count > icl::kQcMaxJobs) return fail(-1, "qchain_wgrad: bad argument");
  icl::QcWgradJobs j;
  memset(&j, 0, sizeof(j));
  long most = 0;
  for (int e = 0; e < count; ++e) {
    if (!g[e] || !x[e] || !dw[e] || rows[e] < 1 || k[e] < 1 || (kind[e] == 0 && (n[e] < 1 || k[e] % 4))) return fail(-1, "qchain_wgrad: bad job");
    j.g[e] = (const float*)g[e]; j.x[e] = (const float*)x[e]; j.dw[e] = (float*)dw[e]; j.db[e] = db ? (float*)db[e] : nullptr;
    j.R[e] = rows[e]; j.N[e] = n[e]; j.K[e] = k[e]; j.kind[e] = kind[e];
    const long items = kind[e] == 1 ? k[e] : (long)n[e] * (k[e] / 4);
    if (items > most) most = items;
  }
  ICL_LAUNCH(icl::qc_wgrad_kernel, dim3(grid_for(most, 256, 1024), count), dim3(256), 0, (hipStream_t)stream, j);
  return check_launch("qc_wgrad");
}

// ---------------------------------------------------------------- validation Dice / HD95 counts and order statistics (kernels/metrics.h)
namespace {

struct SegWs {
  unsigned* cnt; int* box; unsigned* flags; unsigned* hist; unsigned char* bp; unsigned char* bg; int* da; int* db;
  int64_t zero_bytes, total;
};

// carves a workspace into buffers that start at multiples of 256 bytes; a null base only adds the sizes up (the *_ws_bytes queries)
struct WsCarver {
  char* base; int64_t off;
  template <typename T>
  T* take(int64_t bytes) { char* p = base ? base + off : nullptr; off += (bytes + 255) / 256 * 256; return (T*)p; }
};

SegWs seg_layout(char* base, int n0, int n1, int n2, int nc) {
  SegWs w{};
  const int64_t v = (int64_t)n0 * n1 * n2;
  const int64_t nbins = (int64_t)(n0 - 1) * (n0 - 1) + (int64_t)(n1 - 1) * (n1 - 1) + (int64_t)(n2 - 1) * (n2 - 1) + 1;
  WsCarver c{base, 0};
  w.cnt = c.take<unsigned>((int64_t)nc * icl::kSegCnt * 4);
  w.flags = c.take<unsigned>((int64_t)2 * nc * (n0 + n1 + n2) * 4);
  w.hist = c.take<unsigned>(nbins * 4);
  w.zero_bytes = c.off;                     // counters, presence flags and histogram start at zero
  w.box = c.take<int>((int64_t)nc * 16 * 4);
  w.bp = c.take<unsigned char>(v);
  w.bg = c.take<unsigned char>(v);
  w.da = c.take<int>(v * 4);
  w.db = c.take<int>(v * 4);
  w.total = c.off;
  return w;
}

bool seg_shape_ok(int n0, int n1, int n2, int nc) {
  if (n0 < 1 || n1 < 1 || n2 < 1 || nc < 2 || nc > icl::kSegMaxClasses) return false;
  const int64_t v = (int64_t)n0 * n1 * n2;
  const int64_t nbins = (int64_t)(n0 - 1) * (n0 - 1) + (int64_t)(n1 - 1) * (n1 - 1) + (int64_t)(n2 - 1) * (n2 - 1) + 1;
  return v <= 0x7fffffffLL && nbins < (int64_t)icl::kSegInf;      // 32-bit counters and squared distances
}

// the ABI's label element size -> the element type: f(T()) with T = uint8_t (1: uint8 / bool) or long long (8: int64); false, and no
// call, for any other size
template <typename F>
bool seg_label_dispatch(int elem_size, F&& f) {
  switch (elem_size) {
    case 1: f(uint8_t()); return true;
    case 8: f((long long)0); return true;
    default: return false;
  }
}

// the border stage both metric entry points start with; false (nothing launched) for a label element size that is not 1 or 8
bool seg_border_launch(const void* pred, int pred_dtype, const void* gt, int gt_dtype, unsigned char* bp, unsigned char* bg, unsigned* cnt,
                       unsigned* flags, int n0, int n1, int n2, int nc, int all_border, hipStream_t st) {
  bool ok = false;
  seg_label_dispatch(pred_dtype, [&](auto tp) {
    ok = seg_label_dispatch(gt_dtype, [&](auto tg) {
      using TP = decltype(tp);
      using TG = decltype(tg);
      ICL_LAUNCH((icl::seg_border_kernel<TP, TG>), dim3(grid_for((long)n0 * n1 * n2, 256)), dim3(256), 0, st, (const TP*)pred, (const TG*)gt,
                 bp, bg, cnt, flags, n0, n1, n2, nc, all_border);
    });
  });
  return ok;
}

}  // namespace

extern "C" {

int64_t icl_seg_metrics_ws_bytes(int n0, int n1, int n2, int num_classes) {
  if (!seg_shape_ok(n0, n1, n2, num_classes)) return -1;
  return seg_layout(nullptr, n0, n1, n2, num_classes).total;
}

int icl_seg_metrics(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int n0, int n1, int n2, int num_classes, int all_border,
                    int64_t* out, void* ws, void* stream) {
  if (!pred || !gt || !out || !ws || !seg_shape_ok(n0, n1, n2, num_classes))
    return fail(-1, "seg_metrics: bad argument (2 <= num_classes <= %d, n0 n1 n2 <= 2^31 - 1 voxels, workspace of icl_seg_metrics_ws_bytes)",
                icl::kSegMaxClasses);
  const int nc = num_classes;
  hipStream_t st = (hipStream_t)stream;
  const SegWs w = seg_layout((char*)ws, n0, n1, n2, nc);
  ICL_MEMSET_ASYNC(ws, 0, (size_t)w.zero_bytes, st);
  if (!seg_border_launch(pred, pred_dtype, gt, gt_dtype, w.bp, w.bg, w.cnt, w.flags, n0, n1, n2, nc, all_border ? 1 : 0, st))
    return fail(-1, "seg_metrics: label element size must be 1 (uint8) or 8 (int64)");
  if (int e = check_launch("seg_border")) return e;
  ICL_LAUNCH(icl::seg_bbox_kernel, dim3(nc), dim3(256), 0, st, (const unsigned*)w.cnt, (const unsigned*)w.flags, w.box, n0, n1, n2, nc);
  if (int e = check_launch("seg_bbox")) return e;
  const dim3 grid(grid_for((long)n0 * n1 * n2, 256));      // enough for the largest region; workgroups past a class's region exit at once
  for (int k = 1; k < nc; ++k) {
    for (int dir = 0; dir < 2; ++dir) {      // 0: distances from dP to dG (features dG, queries dP); 1: the other way round
      const unsigned char* feat = dir ? w.bp : w.bg;
      const unsigned char* query = dir ? w.bg : w.bp;
      ICL_LAUNCH(icl::seg_edt_axis2_kernel, grid, dim3(256), 0, st, feat, (const int*)w.box, w.da, k, dir, n1, n2);
      ICL_LAUNCH(icl::seg_edt_axis1_kernel, grid, dim3(256), 0, st, (const int*)w.da, (const int*)w.box, w.db, k, dir);
      ICL_LAUNCH(icl::seg_edt_axis0_hist_kernel, grid, dim3(256), 0, st, (const int*)w.db, query, (const int*)w.box, w.hist, k, dir, n1, n2);
    }
    ICL_LAUNCH(icl::seg_select_kernel, dim3(1), dim3(icl::kSegSelectThreads), 0, st, (const unsigned*)w.cnt, (const int*)w.box, w.hist,
               (long long*)out, k);
    if (int e = check_launch("seg_edt / seg_select")) return e;
  }
  return 0;
}

}  // extern "C"

// ---- surface metrics with a voxel spacing: HD95 / HD / ASD / ASSD / NSD in the spacing's units (kernels/metrics_surface.h)
namespace {

struct SurfWs {
  unsigned* cnt; unsigned* flags; unsigned* hist; int* box; icl::SurfSel* state; double* psum; double* pmax; unsigned* pcnt;
  unsigned char* bp; unsigned char* bg; double* ta; double* tb; double* dense[2];
  int64_t zero_bytes, total;
};

SurfWs surf_layout(char* base, int n0, int n1, int n2, int nc) {
  SurfWs w{};
  const int64_t v = (int64_t)n0 * n1 * n2;
  WsCarver c{base, 0};
  w.cnt = c.take<unsigned>((int64_t)nc * icl::kSegCnt * 4);
  w.flags = c.take<unsigned>((int64_t)2 * nc * (n0 + n1 + n2) * 4);
  w.hist = c.take<unsigned>((int64_t)icl::kSurfPasses * 2 * icl::kSurfBins * 4);
  w.zero_bytes = c.off;                     // counters, presence flags and histograms start at zero
  w.box = c.take<int>((int64_t)nc * 16 * 4);
  w.state = c.take<icl::SurfSel>((int64_t)icl::kSurfPasses * sizeof(icl::SurfSel));
  w.psum = c.take<double>((int64_t)2 * icl::kSurfMaxParts * 8);
  w.pmax = c.take<double>((int64_t)2 * icl::kSurfMaxParts * 8);
  w.pcnt = c.take<unsigned>((int64_t)2 * icl::kSurfMaxParts * 4);
  w.bp = c.take<unsigned char>(v);
  w.bg = c.take<unsigned char>(v);
  w.ta = c.take<double>(v * 8);             // axis-2 pass: F0 x F1 x Q2 <= V
  w.tb = c.take<double>(v * 8);             // axis-1 pass: F0 x Q1 x Q2 <= V
  w.dense[0] = c.take<double>(v * 8);       // squared distances of dP to dG over the box of dP
  w.dense[1] = c.take<double>(v * 8);       // ... of dG to dP over the box of dG
  w.total = c.off;
  return w;
}

bool surf_shape_ok(int n0, int n1, int n2, int nc) {
  if (n0 < 1 || n1 < 1 || n2 < 1 || nc < 2 || nc > icl::kSegMaxClasses) return false;
  return (int64_t)n0 * n1 * n2 <= 0x7fffffffLL;      // 32-bit counters
}

template <int PASS>
void surf_radix_launch(const SurfWs& w, dim3 grid, int k, hipStream_t st) {
  ICL_LAUNCH((icl::surf_radix_kernel<PASS>), grid, dim3(icl::kSurfThreads), 0, st, (const double*)w.dense[0], (const double*)w.dense[1],
             (const unsigned*)w.cnt, (const int*)w.box, w.hist, w.state, k);
}

inline bool surf_positive_finite(double v) { return v > 0.0 && v <= 1.7976931348623157e308; }      // false for NaN and infinity

}  // namespace

extern "C" {

int64_t icl_seg_surface_ws_bytes(int n0, int n1, int n2, int num_classes) {
  if (!surf_shape_ok(n0, n1, n2, num_classes)) return -1;
  return surf_layout(nullptr, n0, n1, n2, num_classes).total;
}

int icl_seg_surface_metrics(const void* pred, int pred_dtype, const void* gt, int gt_dtype, int n0, int n1, int n2, int num_classes, double s0,
                            double s1, double s2, double tolerance, int64_t* counts, double* values, void* ws, void* stream) {
  if (!pred || !gt || !counts || !values || !ws || !surf_shape_ok(n0, n1, n2, num_classes))
    return fail(-1, "seg_surface_metrics: bad argument (2 <= num_classes <= %d, n0 n1 n2 <= 2^31 - 1 voxels, workspace of icl_seg_surface_ws_bytes)",
                icl::kSegMaxClasses);
  if (!surf_positive_finite(s0) || !surf_positive_finite(s1) || !surf_positive_finite(s2))
    return fail(-1, "seg_surface_metrics: the spacing must be three finite positive numbers, got (%g, %g, %g)", s0, s1, s2);
  if (!(tolerance >= 0.0) || !(tolerance <= 1.7976931348623157e308))
    return fail(-1, "seg_surface_metrics: the tolerance must be finite and not negative, got %g", tolerance);
  if (pred_dtype != 1 && pred_dtype != 8) return fail(-1, "seg_surface_metrics: label element size must be 1 (uint8) or 8 (int64)");
  if (gt_dtype != 1 && gt_dtype != 8) return fail(-1, "seg_surface_metrics: label element size must be 1 (uint8) or 8 (int64)");
  const int nc = num_classes;
  hipStream_t st = (hipStream_t)stream;
  const SurfWs w = surf_layout((char*)ws, n0, n1, n2, nc);
  const double tau2 = tolerance * tolerance;
  ICL_MEMSET_ASYNC(ws, 0, (size_t)w.zero_bytes, st);
  // the first stage is the integer path's: same kernels, same instantiations
  (void)seg_border_launch(pred, pred_dtype, gt, gt_dtype, w.bp, w.bg, w.cnt, w.flags, n0, n1, n2, nc, 0, st);      // sizes checked above
  if (int e = check_launch("seg_border")) return e;
  ICL_LAUNCH(icl::seg_bbox_kernel, dim3(nc), dim3(256), 0, st, (const unsigned*)w.cnt, (const unsigned*)w.flags, w.box, n0, n1, n2, nc);
  if (int e = check_launch("seg_bbox")) return e;
  const long v = (long)n0 * n1 * n2;
  const dim3 grid(grid_for(v, 256));      // enough for the largest region; workgroups past a class's region do nothing
  const int parts = grid_for(v, icl::kSurfThreads, icl::kSurfMaxParts);
  const dim3 rgrid(grid_for(2 * v, icl::kSurfThreads, 2048));      // the select reads both dense buffers
  for (int k = 1; k < nc; ++k) {
    for (int dir = 0; dir < 2; ++dir) {      // 0: distances from dP to dG (features dG, queries dP); 1: the other way round
      const unsigned char* feat = dir ? w.bp : w.bg;
      const unsigned char* query = dir ? w.bg : w.bp;
      ICL_LAUNCH(icl::surf_edt_axis2_kernel, grid, dim3(256), 0, st, feat, (const int*)w.box, w.ta, k, dir, n1, n2, s2);
      ICL_LAUNCH(icl::surf_edt_axis1_kernel, grid, dim3(256), 0, st, (const double*)w.ta, (const int*)w.box, w.tb, k, dir, s1);
      ICL_LAUNCH(icl::surf_edt_axis0_kernel, grid, dim3(256), 0, st, (const double*)w.tb, query, (const int*)w.box, w.dense[dir], k, dir, n1, n2, s0);
      ICL_LAUNCH(icl::surf_reduce_kernel, dim3(parts), dim3(icl::kSurfThreads), 0, st, (const double*)w.dense[dir], (const int*)w.box,
                 w.psum + dir * icl::kSurfMaxParts, w.pmax + dir * icl::kSurfMaxParts, w.pcnt + dir * icl::kSurfMaxParts, k, dir, tau2);
    }
    surf_radix_launch<0>(w, rgrid, k, st);
    surf_radix_launch<1>(w, rgrid, k, st);
    surf_radix_launch<2>(w, rgrid, k, st);
    surf_radix_launch<3>(w, rgrid, k, st);
    surf_radix_launch<4>(w, rgrid, k, st);
    surf_radix_launch<5>(w, rgrid, k, st);
    ICL_LAUNCH(icl::surf_finish_kernel, dim3(1), dim3(icl::kSurfThreads), 0, st, (const unsigned*)w.cnt, (const int*)w.box, w.hist,
               (const icl::SurfSel*)w.state, (const double*)w.psum, (const double*)w.pmax, (const unsigned*)w.pcnt, parts, (long long*)counts,
               values, k);
    if (int e = check_launch("surf_edt / surf_radix / surf_finish")) return e;
  }
  return 0;
}

}  // extern "C"

// ---- connected components of a label map and the keep-largest / minimum-size filter (kernels/components.h)
namespace {

struct CcWs {
  int* parent; int* size; int* labels; unsigned long long* pkey; int* pcnt; long long* rec;
  int64_t total;
};

CcWs cc_layout(char* base, int n0, int n1, int n2) {
  CcWs w{};
  const int64_t v = (int64_t)n0 * n1 * n2;
  WsCarver c{base, 0};
  w.parent = c.take<int>(v * 4);
  w.size = c.take<int>(v * 4);
  w.labels = c.take<int>(v * 4);            // the filter's labels (icl_seg_components writes the caller's)
  w.pkey = c.take<unsigned long long>((int64_t)icl::kCcMaxParts * icl::kSegMaxClasses * 8);
  w.pcnt = c.take<int>((int64_t)icl::kCcMaxParts * icl::kSegMaxClasses * 4);
  w.rec = c.take<long long>((int64_t)icl::kSegMaxClasses * icl::kCcRec * 8);
  w.total = c.off;
  return w;
}

bool cc_shape_ok(int n0, int n1, int n2, int nc) {
  return seg_shape_ok(n0, n1, n2, nc) && (int64_t)n0 * n1 * n2 + 1 <= 0x7fffffffLL;      // a label is 1 + a voxel index, in an int32
}

template <typename T, int CONN>
void cc_label_launch(const void* map, const CcWs& w, int* labels, long long* counts, int n0, int n1, int n2, int nc, hipStream_t st) {
  const long v = (long)n0 * n1 * n2;
  const int nt0 = (n0 + icl::kCcT0 - 1) / icl::kCcT0, nt1 = (n1 + icl::kCcT1 - 1) / icl::kCcT1, nt2 = (n2 + icl::kCcT2 - 1) / icl::kCcT2;
  const dim3 grid(grid_for(v, 256));
  const int parts = grid_for(v, icl::kCcThreads, icl::kCcMaxParts);
  ICL_LAUNCH((icl::cc_tile_kernel<T, CONN>), dim3((unsigned)((long)nt0 * nt1 * nt2)), dim3(icl::kCcThreads), 0, st, (const T*)map, w.parent,
             w.size, n0, n1, n2, nc, nt1, nt2);
  ICL_LAUNCH((icl::cc_merge_kernel<T, CONN>), grid, dim3(256), 0, st, (const T*)map, w.parent, n0, n1, n2, nc);
  ICL_LAUNCH(icl::cc_flatten_kernel, grid, dim3(256), 0, st, (const int*)w.parent, labels, w.size, v);
  ICL_LAUNCH((icl::cc_reduce_kernel<T>), dim3(parts), dim3(icl::kCcThreads), 0, st, (const T*)map, (const int*)labels, (const int*)w.size,
             w.pkey, w.pcnt, v, nc);
  ICL_LAUNCH(icl::cc_finish_kernel, dim3(1), dim3(icl::kCcThreads), 0, st, (const unsigned long long*)w.pkey, (const int*)w.pcnt, parts,
             w.rec, counts, nc);
}

template <typename T>
void cc_label_dispatch(const void* map, const CcWs& w, int* labels, long long* counts, int n0, int n1, int n2, int nc, int connectivity,
                       hipStream_t st) {
  switch (connectivity) {
    case 1: cc_label_launch<T, 1>(map, w, labels, counts, n0, n1, n2, nc, st); break;
    case 2: cc_label_launch<T, 2>(map, w, labels, counts, n0, n1, n2, nc, st); break;
    default: cc_label_launch<T, 3>(map, w, labels, counts, n0, n1, n2, nc, st);
  }
}

// the checks both entry points share; 0 when the arguments are fine
int cc_check(const char* who, const void* map, int dtype, int n0, int n1, int n2, int nc, int connectivity, const void* ws) {
  if (!map || !ws || !cc_shape_ok(n0, n1, n2, nc))
    return fail(-1, "%s: bad argument (2 <= num_classes <= %d, n0 n1 n2 <= 2^31 - 2 voxels, workspace of icl_seg_components_ws_bytes)", who,
                icl::kSegMaxClasses);
  if (connectivity < 1 || connectivity > 3) return fail(-1, "%s: connectivity must be 1, 2 or 3, got %d", who, connectivity);
  if (dtype != 1 && dtype != 8) return fail(-1, "%s: label element size must be 1 (uint8) or 8 (int64)", who);
  return 0;
}

}  // namespace

extern "C" {

int64_t icl_seg_components_ws_bytes(int n0, int n1, int n2, int num_classes) {
  if (!cc_shape_ok(n0, n1, n2, num_classes)) return -1;
  return cc_layout(nullptr, n0, n1, n2).total;
}

int icl_seg_components(const void* map, int dtype, int n0, int n1, int n2, int num_classes, int connectivity, int32_t* labels, int64_t* counts,
                       void* ws, void* stream) {
  if (int e = cc_check("seg_components", map, dtype, n0, n1, n2, num_classes, connectivity, ws)) return e;
  if (!labels || !counts) return fail(-1, "seg_components: labels and counts must not be null");
  hipStream_t st = (hipStream_t)stream;
  const CcWs w = cc_layout((char*)ws, n0, n1, n2);
  seg_label_dispatch(dtype, [&](auto t) {
    cc_label_dispatch<decltype(t)>(map, w, labels, (long long*)counts, n0, n1, n2, num_classes, connectivity, st);
  });
  return check_launch("cc_tile / cc_merge / cc_flatten / cc_reduce / cc_finish");
}

int icl_seg_filter_components(const void* map, int dtype, int n0, int n1, int n2, int num_classes, int connectivity, int keep_largest,
                              int64_t min_size, void* out, int64_t* counts, void* ws, void* stream) {
  if (int e = cc_check("seg_filter_components", map, dtype, n0, n1, n2, num_classes, connectivity, ws)) return e;
  if (!out) return fail(-1, "seg_filter_components: out must not be null");
  if (min_size < 0) return fail(-1, "seg_filter_components: min_size must not be negative, got %lld", (long long)min_size);
  hipStream_t st = (hipStream_t)stream;
  const CcWs w = cc_layout((char*)ws, n0, n1, n2);
  const long v = (long)n0 * n1 * n2;
  const dim3 grid(grid_for(v, 256));
  seg_label_dispatch(dtype, [&](auto t) {
    using T = decltype(t);
    cc_label_dispatch<T>(map, w, w.labels, (long long*)counts, n0, n1, n2, num_classes, connectivity, st);
    ICL_LAUNCH((icl::cc_filter_kernel<T>), grid, dim3(256), 0, st, (const T*)map, (const int*)w.labels, (const int*)w.size,
               (const long long*)w.rec, (T*)out, v, num_classes, keep_largest ? 1 : 0, (long long)min_size);
  });
  return check_launch("cc_tile / cc_merge / cc_flatten / cc_reduce / cc_finish / cc_filter");
}

}  // extern "C"

// ---- 3-D sliding window of the validation loops (kernels/window.h)
namespace {

// origins [n][3] -> kernel arguments; nullptr + message when n, or a window, does not fit
const char* win_batch(const int32_t* origins, int n, int p0, int p1, int p2, int r0, int r1, int r2, icl::WinBatch& wb) {
  static thread_local char msg[160];
  if (n < 1 || n > icl::kWinMaxBatch) {
    snprintf(msg, sizeof(msg), "%d windows (1 <= n <= %d)", n, icl::kWinMaxBatch);
    return msg;
  }
  if (r0 < 1 || r1 < 1 || r2 < 1 || p0 < r0 || p1 < r1 || p2 < r2) {
    snprintf(msg, sizeof(msg), "window %d x %d x %d does not fit the padded extent %d x %d x %d", r0, r1, r2, p0, p1, p2);
    return msg;
  }
  const int pe[3] = {p0, p1, p2}, re[3] = {r0, r1, r2};
  for (int w = 0; w < n; ++w)
    for (int d = 0; d < 3; ++d) {
      const int o = origins[3 * w + d];
      if (o < 0 || o > pe[d] - re[d]) {
        snprintf(msg, sizeof(msg), "window %d: origin %d on axis %d puts it outside the padded extent %d (window %d)", w, o, d, pe[d], re[d]);
        return msg;
      }
      wb.o[w][d] = o;
    }
  return nullptr;
}

// flips [n] -> kernel arguments; nullptr + message when a mask is not a set of the three window axes
const char* win_flips(const int32_t* flips, int n, icl::WinFlips& fl) {
  static thread_local char msg[96];
  for (int w = 0; w < n; ++w) {
    if (flips[w] < 0 || flips[w] > 7) {
      snprintf(msg, sizeof(msg), "window %d: mirror mask %d (0 <= mask <= 7)", w, flips[w]);
      return msg;
    }
    fl.m |= (unsigned long long)flips[w] << (4 * w);
  }
  return nullptr;
}

inline bool win_pads_ok(int s0, int s1, int s2, int a0, int a1, int a2, int p0, int p1, int p2) {
  return s0 >= 1 && s1 >= 1 && s2 >= 1 && a0 >= 0 && a1 >= 0 && a2 >= 0 && (long)a0 + s0 <= p0 && (long)a1 + s1 <= p1 && (long)a2 + s2 <= p2;
}

constexpr int kWinMaxWgs = 2048;

template <int NCMAX>
void win_accumulate_launch(bool quad, dim3 grid, hipStream_t st, const float* logits, const float* imp, float* score, float* weight,
                           const icl::WinBatch& wb, const icl::WinFlips* fl, int n, int c, icl::WinExt p, icl::WinExt r, icl::WinExt lo,
                           icl::WinExt ext, int softmax) {
  if (fl) {
    if (quad) {
      ICL_LAUNCH((icl::window_accumulate_kernel<NCMAX, 4, icl::WinFlips>), grid, dim3(256), 0, st, logits, imp, score, weight, wb, n, c, p, r, lo, ext, softmax, *fl);
    } else {
      ICL_LAUNCH((icl::window_accumulate_kernel<NCMAX, 1, icl::WinFlips>), grid, dim3(256), 0, st, logits, imp, score, weight, wb, n, c, p, r, lo, ext, softmax, *fl);
    }
  } else if (quad) {
    ICL_LAUNCH((icl::window_accumulate_kernel<NCMAX, 4>), grid, dim3(256), 0, st, logits, imp, score, weight, wb, n, c, p, r, lo, ext, softmax);
  } else {
    ICL_LAUNCH((icl::window_accumulate_kernel<NCMAX, 1>), grid, dim3(256), 0, st, logits, imp, score, weight, wb, n, c, p, r, lo, ext, softmax);
  }
}

// icl_window_gather (flips == nullptr) and icl_window_gather_flipped: one set of refusals, one grid, the kernel of the form asked for
int win_gather(const char* who, const float* vol, float* out, const int32_t* origins, const int32_t* flips, bool flipped, int n, int cin,
               int s0, int s1, int s2, int a0, int a1, int a2, int p0, int p1, int p2, int r0, int r1, int r2, void* stream) {
  if (!vol || !out || !origins || (flipped && !flips)) return fail(-1, "%s: null pointer", who);
  if (cin < 1 || !win_pads_ok(s0, s1, s2, a0, a1, a2, p0, p1, p2))
    return fail(-1, "%s: bad extents (Cin %d, volume %d x %d x %d at %d, %d, %d of %d x %d x %d)", who, cin, s0, s1, s2, a0, a1, a2, p0, p1, p2);
  icl::WinBatch wb{};
  icl::WinFlips fl{};
  if (const char* m = win_batch(origins, n, p0, p1, p2, r0, r1, r2, wb)) return fail(-1, "%s: %s", who, m);
  if (flipped)
    if (const char* m = win_flips(flips, n, fl)) return fail(-1, "%s: %s", who, m);
  const icl::WinExt s{s0, s1, s2}, a{a0, a1, a2}, r{r0, r1, r2};
  const bool quad = (r2 & 3) == 0 && aligned16(vol) && aligned16(out);
  const long total = (long)cin * r0 * r1 * (quad ? r2 / 4 : r2);
  const dim3 grid(grid_for(total, 256, kWinMaxWgs / n > 0 ? kWinMaxWgs / n : 1), n);
  if (flipped) {
    if (quad) {
      ICL_LAUNCH((icl::window_gather_kernel<4, icl::WinFlips>), grid, dim3(256), 0, (hipStream_t)stream, vol, out, wb, cin, s, a, r, fl);
    } else {
      ICL_LAUNCH((icl::window_gather_kernel<1, icl::WinFlips>), grid, dim3(256), 0, (hipStream_t)stream, vol, out, wb, cin, s, a, r, fl);
    }
  } else if (quad) {
    ICL_LAUNCH(icl::window_gather_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, vol, out, wb, cin, s, a, r);
  } else {
    ICL_LAUNCH(icl::window_gather_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, vol, out, wb, cin, s, a, r);
  }
  return check_launch(who);
}

int win_accumulate(const char* who, const float* logits, const float* importance, float* score, float* weight, const int32_t* origins,
                   const int32_t* flips, bool flipped, int n, int c, int p0, int p1, int p2, int r0, int r1, int r2, int softmax, void* stream) {
  if (!logits || !score || !weight || !origins || (flipped && !flips)) return fail(-1, "%s: null pointer", who);
  if (c < 1 || c > icl::kWinMaxClasses) return fail(-1, "%s: %d classes (1 <= C <= %d)", who, c, icl::kWinMaxClasses);
  icl::WinBatch wb{};
  icl::WinFlips fl{};
  if (const char* m = win_batch(origins, n, p0, p1, p2, r0, r1, r2, wb)) return fail(-1, "%s: %s", who, m);
  if (flipped)
    if (const char* m = win_flips(flips, n, fl)) return fail(-1, "%s: %s", who, m);
  const icl::WinExt p{p0, p1, p2}, r{r0, r1, r2};
  int lo[3], hi[3];
  bool quad = (p2 & 3) == 0 && (r2 & 3) == 0 && aligned16(logits) && aligned16(score) && aligned16(weight) && (!importance || aligned16(importance));
  for (int d = 0; d < 3; ++d) { lo[d] = wb.o[0][d]; hi[d] = wb.o[0][d]; }
  for (int w = 0; w < n; ++w) {
    for (int d = 0; d < 3; ++d) {
      if (wb.o[w][d] < lo[d]) lo[d] = wb.o[w][d];
      if (wb.o[w][d] > hi[d]) hi[d] = wb.o[w][d];
    }
    if (wb.o[w][2] & 3) quad = false;
  }
  const icl::WinExt l{lo[0], lo[1], lo[2]}, ext{hi[0] - lo[0] + r0, hi[1] - lo[1] + r1, hi[2] - lo[2] + r2};      // the batch's bounding box
  const long total = (long)ext.d0 * ext.d1 * (quad ? ext.d2 / 4 : ext.d2);
  const dim3 grid(grid_for(total, 256, kWinMaxWgs));
  hipStream_t st = (hipStream_t)stream;
  const int sm = softmax ? 1 : 0;
  const icl::WinFlips* flp = flipped ? &fl : nullptr;
  if (c <= 4) win_accumulate_launch<4>(quad, grid, st, logits, importance, score, weight, wb, flp, n, c, p, r, l, ext, sm);
  else if (c <= 16) win_accumulate_launch<16>(quad, grid, st, logits, importance, score, weight, wb, flp, n, c, p, r, l, ext, sm);
  else win_accumulate_launch<0>(quad, grid, st, logits, importance, score, weight, wb, flp, n, c, p, r, l, ext, sm);
  return check_launch(who);
}

}  // namespace

extern "C" {

int icl_window_gather(const float* vol, float* out, const int32_t* origins, int n, int cin, int s0, int s1, int s2, int a0, int a1, int a2,
                      int p0, int p1, int p2, int r0, int r1, int r2, void* stream) {
  return win_gather("window_gather", vol, out, origins, nullptr, false, n, cin, s0, s1, s2, a0, a1, a2, p0, p1, p2, r0, r1, r2, stream);
}

int icl_window_gather_flipped(const float* vol, float* out, const int32_t* origins, const int32_t* flips, int n, int cin, int s0, int s1,
                              int s2, int a0, int a1, int a2, int p0, int p1, int p2, int r0, int r1, int r2, void* stream) {
  return win_gather("window_gather_flipped", vol, out, origins, flips, true, n, cin, s0, s1, s2, a0, a1, a2, p0, p1, p2, r0, r1, r2, stream);
}

int icl_window_accumulate(const float* logits, const float* importance, float* score, float* weight, const int32_t* origins, int n, int c,
                          int p0, int p1, int p2, int r0, int r1, int r2, int softmax, void* stream) {
  return win_accumulate("window_accumulate", logits, importance, score, weight, origins, nullptr, false, n, c, p0, p1, p2, r0, r1, r2, softmax,
                        stream);
}

int icl_window_accumulate_flipped(const float* logits, const float* importance, float* score, float* weight, const int32_t* origins,
                                  const int32_t* flips, int n, int c, int p0, int p1, int p2, int r0, int r1, int r2, int softmax,
                                  void* stream) {
  return win_accumulate("window_accumulate_flipped", logits, importance, score, weight, origins, flips, true, n, c, p0, p1, p2, r0, r1, r2,
                        softmax, stream);
}

int icl_window_finalize(const float* score, const float* weight, int64_t* label, float* quotients, int c, int p0, int p1, int p2, int a0,
                        int a1, int a2, int s0, int s1, int s2, void* stream) {
  if (!score || !weight || (!label && !quotients)) return fail(-1, "window_finalize: null pointer");
  if (quotients == score && (s0 != p0 || s1 != p1 || s2 != p2))
    return fail(-1, "window_finalize: the quotients can replace the score map only where nothing is cropped");
  if (c < 1 || c > icl::kWinMaxClasses) return fail(-1, "window_finalize: %d classes (1 <= C <= %d)", c, icl::kWinMaxClasses);
  if (!win_pads_ok(s0, s1, s2, a0, a1, a2, p0, p1, p2))
    return fail(-1, "window_finalize: bad extents (volume %d x %d x %d at %d, %d, %d of %d x %d x %d)", s0, s1, s2, a0, a1, a2, p0, p1, p2);
  const icl::WinExt p{p0, p1, p2}, a{a0, a1, a2}, s{s0, s1, s2};
  const bool quad = (s2 & 3) == 0 && (p2 & 3) == 0 && (a2 & 3) == 0 && aligned16(score) && aligned16(weight) && (!label || aligned16(label)) &&
                    (!quotients || aligned16(quotients));
  const dim3 grid(grid_for((long)s0 * s1 * (quad ? s2 / 4 : s2), 256, kWinMaxWgs));
  if (quad) {
    ICL_LAUNCH(icl::window_finalize_kernel<4>, grid, dim3(256), 0, (hipStream_t)stream, score, weight, (long long*)label, quotients, c, p, a, s);
  } else {
    ICL_LAUNCH(icl::window_finalize_kernel<1>, grid, dim3(256), 0, (hipStream_t)stream, score, weight, (long long*)label, quotients, c, p, a, s);
  }
  return check_launch("window_finalize");
}

// ---- live batch (DESIGN.md §4.4 "Live batch"): a gradient whose samples [n_live, n) are exactly zero.  Every `_live` sibling computes samples
// [0, n_live) exactly as its entry point does when called with n = n_live on the same pointers and batch strides (all of these operators
// are per sample, and samples are the outermost index of every tensor, dropout-mask index and tile list), and writes zeros to samples
// [n_live, n) of every output gradient in the same call on the same stream (a fill node under capture).  n_live == n: the entry point itself.

namespace {
inline int live_args(int n, int n_live, const char* who) {
  if (n < 1 || n_live < 1 || n_live > n) return fail(-1, "%s: bad live batch (1 <= n_live <= n)", who);
  return 0;
}
// zeros to samples [n_live, n) of a dense [n][elems] gradient
inline int live_zero_tail(float* p, int n, int n_live, int64_t elems, hipStream_t st, const char* who) {
  if (n_live >= n) return 0;
  ICL_MEMSET_ASYNC(p + (size_t)n_live * elems, 0, (size_t)(n - n_live) * elems * sizeof(float), st);
  char what[96];
  snprintf(what, sizeof(what), "%s: tail", who);
  return check_launch(what);
}
// the live forms of the forward entry points: `call(n_live)` is the entry point on the live samples; then the record of its kernel and
// the zero tail.  1 from the call: nothing launched (the caller takes the fp32 pack), nothing zeroed.
extern "C++" template <class Call>
int live_fwd(const char* who, float* y, int n, int n_live, int64_t dense, int64_t y_bstride, void* stream, Call call) {
  if (int rc = live_args(n, n_live, who)) return rc;
  if (n_live < n && y_bstride != dense) return fail(-1, "%s: y must be dense", who);
  if (int rc = call(n_live)) return rc;
  snprintf(g_kernel_live_fwd, sizeof(g_kernel_live_fwd), "%s", g_kernel);
  return live_zero_tail(y, n, n_live, y_bstride, (hipStream_t)stream, who);
}
}  // namespace

// 1: the 3^3 planner plans a batch of n_live as it plans a batch of n — split-product kernels, nothing split over the channel chunks
// (the deep levels' split count follows the batch size: their sums would re-associate) — so the live samples come out bit for bit.
// Rows of 12 voxels and the 6^3 volume run on the split-product kernels only when split, else on the fp32 kernels, whose split does
// follow the batch size: refused.  Not mirrored: operands that are not 16-byte aligned (a real call then falls to the fp32 kernels; the
// samples stay correct, their last bits may differ from the full call's).
int icl_conv3d_fwd_live_ok(int n, int n_live, int cin, int cout, int d, int h, int w) {
  if (n < 1 || n_live < 1 || n_live > n || cin < 1 || cout < 1 || d < 1 || h < 1 || w < 1) return 0;
  if (w == icl::Bf3F12::TX || (w == 6 && h == 6 && d == 6)) return 0;
  const ConvEnv e = conv_env();
  const int batches[2] = {n, n_live};
  for (const int batch : batches) {
    const SplitPlan p = plan_conv_split({batch, cin, cout, d, h, w}, e);
    if (!p.ok || p.ksplit > 1) return 0;
  }
  return 1;
}

const char* icl_last_live_fwd_kernel_name(void) { return g_kernel_live_fwd; }
void icl_last_wgrad_grid(int32_t* launched, int32_t* planned) {
  if (launched) *launched = g_wgrad_grid[0];
  if (planned) *planned = g_wgrad_grid[1];
}

int icl_conv3d_fwd_presplit_live(const float* x, const void* wsplit, const float* bias, float* y, int n, int n_live, int cin, int cout, int d,
                                 int h, int w, int64_t x_bstride, int64_t y_bstride, void* stream) {
  return live_fwd("conv3d_fwd_presplit_live", y, n, n_live, (int64_t)cout * d * h * w, y_bstride, stream, [&](int nl) {
    return icl_conv3d_fwd_presplit(x, wsplit, bias, y, nl, cin, cout, d, h, w, x_bstride, y_bstride, stream); });
}

int icl_conv3d_fwd_presplit_ws_live(const float* x, const void* wsplit, const float* bias, float* y, void* ws, int n, int n_live, int cin,
                                    int cout, int d, int h, int w, int64_t x_bstride, int64_t y_bstride, void* stream) {
  return live_fwd("conv3d_fwd_presplit_ws_live", y, n, n_live, (int64_t)cout * d * h * w, y_bstride, stream, [&](int nl) {
    return icl_conv3d_fwd_presplit_ws(x, wsplit, bias, y, ws, nl, cin, cout, d, h, w, x_bstride, y_bstride, stream); });
}

int icl_conv3d_fwd_live(const float* x, const float* wp, const float* bias, float* y, void* ws, int n, int n_live, int cin, int cout, int d,
                        int h, int w, int ks, int64_t x_bstride, int64_t y_bstride, void* stream) {
  return live_fwd("conv3d_fwd_live", y, n, n_live, (int64_t)cout * d * h * w, y_bstride, stream, [&](int nl) {
    return icl_conv3d_fwd(x, wp, bias, y, ws, nl, cin, cout, d, h, w, ks, x_bstride, y_bstride, stream); });
}

// The weight gradient has no per-sample output.  Its live form keeps the launch plan of the batch of n and skips the workgroups that own
// no live tile (wgrad_live_prefix): same slabs, same order, bit-identical sums.  Workspace as for n.
int64_t icl_conv3d_wgrad_ws_bytes_live(int n, int n_live, int cin, int cout, int ks) {
  if (n < 1 || n_live < 1 || n_live > n) return 0;
  return icl_conv3d_wgrad_ws_bytes(n, cin, cout, ks);
}

int icl_conv3d_wgrad_live(const float* x, const float* gy, float* gw, float* gbias, void* ws, int n, int n_live, int cin, int cout, int d,
                          int h, int w, int ks, int64_t x_bstride, int64_t gy_bstride, void* stream) {
  if (int rc = live_args(n, n_live, "conv3d_wgrad_live")) return rc;
  return wgrad_run(x, gy, gw, gbias, ws, n, n_live, cin, cout, d, h, w, ks, x_bstride, gy_bstride, stream);
}

int icl_conv3d_wgrad_slabs_live(const float* x, const float* gy, void* ws, int n, int n_live, int cin, int cout, int d, int h, int w, int ks,
                                int64_t x_bstride, int64_t gy_bstride, int32_t* nslabs, void* stream) {
  if (int rc = live_args(n, n_live, "conv3d_wgrad_slabs_live")) return rc;
  return wgrad_slabs_run(x, gy, ws, n, n_live, cin, cout, d, h, w, ks, x_bstride, gy_bstride, nslabs, stream);
}

int icl_norm_bwd_live(const float* gy, const float* x, const float* mean, const float* rstd, const float* gamma, const float* beta, float* gx,
                      float* dgamma, float* dbeta, int n, int n_live, int c, int64_t s, int mode, int use_batch_stats, int act, void* ws,
                      void* stream) {
  if (int rc = live_args(n, n_live, "norm_bwd_live")) return rc;
  // instance statistics without an affine pair only: a batch group (mode 1) couples the samples, and dgamma / dbeta rows are per (n, c)
  if (n_live < n && (mode != 0 || dgamma || dbeta)) return fail(-1, "norm_bwd_live: a live batch needs instance statistics, no affine pair");
  const int rc = icl_norm_bwd(gy, x, mean, rstd, gamma, beta, gx, dgamma, dbeta, n_live, c, s, mode, use_batch_stats, act, ws, stream);
  if (rc) return rc;
  return live_zero_tail(gx, n, n_live, (int64_t)c * s, (hipStream_t)stream, "norm_bwd_live");
}

int icl_trilinear_bwd_live(const float* gy, float* gx, void* ws, int n, int n_live, int c, int di, int hi, int wi, int dout, int hout, int wout,
                           int64_t gy_bstride, int align_corners, void* stream) {
  if (int rc = live_args(n, n_live, "trilinear_bwd_live")) return rc;
  const int rc = icl_trilinear_bwd(gy, gx, ws, n_live, c, di, hi, wi, dout, hout, wout, gy_bstride, align_corners, stream);
  if (rc) return rc;
  return live_zero_tail(gx, n, n_live, (int64_t)c * di * hi * wi, (hipStream_t)stream, "trilinear_bwd_live");
}

int icl_conv1x1_small_live(const float* x, const float* w, const float* bias, float* y, int n, int n_live, int cin, int cout, int64_t s,
                           int w_ostride, int w_istride, void* stream) {
  if (int rc = live_args(n, n_live, "conv1x1_small_live")) return rc;
  if (!x || !w || !y || cin < 1 || cout < 1 || s < 4 || (s & 3)) return fail(-1, "conv1x1_small_live: bad argument (s %% 4 == 0)");
  const int rc = conv1x1_small_run(x, w, bias, y, n_live, cin, cout, s, w_ostride, w_istride, icl::DropSpec{}, (hipStream_t)stream, n);
  if (rc) return rc;
  return live_zero_tail(y, n, n_live, (int64_t)cout * s, (hipStream_t)stream, "conv1x1_small_live");
}

// (the mask is a hash of the element index (b * C + c) * S + v: the live samples are a prefix, their indices and masks are unchanged)
int icl_conv1x1_dropout_live(const float* x, const float* w, const float* bias, float* y, int n, int n_live, int cin, int cout, int64_t s,
                             int w_ostride, int w_istride, int mask_mode, uint32_t seed, float p, const uint32_t* seed_dev, void* stream) {
  if (int rc = live_args(n, n_live, "conv1x1_dropout_live")) return rc;
  if (!x || !w || !y || cin < 1 || cout < 1 || s < 4 || (s & 3) || (mask_mode != 1 && mask_mode != 2) || !(p >= 0.f && p < 1.f))
    return fail(-1, "conv1x1_dropout_live: bad argument");
  const int rc = conv1x1_small_run(x, w, bias, y, n_live, cin, cout, s, w_ostride, w_istride, drop_spec(mask_mode, seed, p, seed_dev),
                                   (hipStream_t)stream, n);
  if (rc) return rc;      // 1: n * s < 65536, nothing launched, nothing zeroed
  return live_zero_tail(y, n, n_live, (int64_t)cout * s, (hipStream_t)stream, "conv1x1_dropout_live");
}

int icl_conv1x1_wgrad_live(const float* x, const float* gy, float* gw, float* gbias, void* ws, int n, int n_live, int cin, int cout, int64_t s,
                           int64_t x_bstride, int64_t gy_bstride, void* stream) {
  if (int rc = live_args(n, n_live, "conv1x1_wgrad_live")) return rc;
  // (the row split of this HBM-bound reduction follows n * s: the whole batch, whose dead rows add exact zeros — bit-identical sums)
  return icl_conv1x1_wgrad(x, gy, gw, gbias, ws, n, cin, cout, s, x_bstride, gy_bstride, stream);
}

int icl_conv1x1_wgrad_dropout_live(const float* x, const float* gy, float* gw, float* gbias, void* ws, int n, int n_live, int cin, int cout,
                                   int64_t s, int64_t gy_bstride, uint32_t seed, float p, const uint32_t* seed_dev, void* stream) {
  if (int rc = live_args(n, n_live, "conv1x1_wgrad_dropout_live")) return rc;
  return icl_conv1x1_wgrad_dropout(x, gy, gw, gbias, ws, n, cin, cout, s, gy_bstride, seed, p, seed_dev, stream);
}

int icl_conv1x1_wgrad_dropout_norm_live(const float* x, const float* ss, const float* gy, float* gw, float* gbias, void* ws, int n, int n_live,
                                        int cin, int cout, int64_t s, int64_t gy_bstride, uint32_t seed, float p, const uint32_t* seed_dev,
                                        void* stream) {
  if (int rc = live_args(n, n_live, "conv1x1_wgrad_dropout_norm_live")) return rc;
  return icl_conv1x1_wgrad_dropout_norm(x, ss, gy, gw, gbias, ws, n, cin, cout, s, gy_bstride, seed, p, seed_dev, stream);
}

}  // extern "C"
