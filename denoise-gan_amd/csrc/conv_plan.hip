// Conv planner (host code only; a .hip file because dgan/build.py compiles csrc/*.hip): which
// kernel, arithmetic, tile and split-K count each op of a layer runs, its workspace layout, and
// which operand planes it reads.  Every measured rule lives here; conv.hip launches the plans.
#include "conv_plan.h"
#include "conv_tiles.h"
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace dg {

// planner tables of the tile lists (conv_tiles.h): fp32 MFMA (launch_gemm), bf16x6
// (launch_gemm_x6), fp16 (launch_gemm_f16: the bf16x6 tiles, K-tile 32), fp16x3 (launch_gemm_x3)
#define DG_ROW(I, BM, BN, WGM, WGN, BK, MINW, NBUF, BPC, EFF) {BM, BN, WGM, WGN, BK, BPC, EFF},
#define DG_ROW_F16(I, BM, BN, WGM, WGN, BK, MINW, NBUF, BPC, EFF) {BM, BN, WGM, WGN, DG_TILES_F16_BK, BPC, EFF},
static const TileCfg kCfgs[] = {DG_TILES_FP32(DG_ROW)};
static const TileCfg kX6Cfgs[] = {DG_TILES_X6(DG_ROW)};
static const TileCfg kF16Cfgs[] = {DG_TILES_X6(DG_ROW_F16)};
static const TileCfg kX3Cfgs[] = {DG_TILES_X3(DG_ROW)};
#undef DG_ROW
#undef DG_ROW_F16

int engine_mode(const dg_conv_desc_s *d, int op) {
    // layer op -> conv-view engine
    if (!d->transpose) return op == DG_OP_FWD ? MODE_FWD : (op == DG_OP_BWD_DATA ? MODE_DGRAD : MODE_WGRAD);
    return op == DG_OP_FWD ? MODE_DGRAD : (op == DG_OP_BWD_DATA ? MODE_FWD : MODE_WGRAD);
}

static bool cfg_vec(const ConvGeom &g, int mode, int bk) {
    if (mode == MODE_FWD) return g.Ci % bk == 0;
    if (mode == MODE_DGRAD) return g.Co % bk == 0;
    return g.Ci % 4 == 0;
}

// Plan features switched off for same-box A/B runs: DG_PLAN_DISABLE is a
// comma-separated list of {shortk, small, co1, tlast, direct, halo, halo2, halo4, halo_f16, xcd_phase, narrow_px, ntile,
// tile32, f16planes, halo32}
// (read when a descriptor is planned; unset in production runs)
bool plan_off(const char *feature) {
    const char *list = getenv("DG_PLAN_DISABLE");
    const size_t n = strlen(feature);
    // (an occurrence of the name that is a whole item of the list)
    for (const char *q = list ? strstr(list, feature) : nullptr; q; q = strstr(q + 1, feature))
        if ((q == list || q[-1] == ',') && (q[n] == ',' || !q[n])) return true;
    return false;
}

// Tile config + split-K count for plan pl (M, N, K, nphase set) from a config
// table; returns the modelled time.  Modelled time of a candidate:
//   rounds x (blocks per CU x per-block MFMA work) / (CU peak x occupancy efficiency)
// + split-K slab traffic, where blocks per CU = min(resident limit, blocks / 256).
template <int ncfg>
static double choose_tiles(OpPlan &pl, const TileCfg (&cfgs)[ncfg], double peak, const char *force_env, int rule = -1) {
    const double cu_flops = peak / 256.0;
    static const double occ_eff[] = {0.0, 0.62, 0.80, 0.88, 0.92};
    int forced = rule;   // (a measured per-shape rule of the caller; the environment overrides it)
    if (const char *f = getenv(force_env)) forced = atoi(f);
    // DG_FORCE_SPLITS: split-K count for sweeps (scripts/diag/deep_sweep.py); unset in production
    long fsplits = 0;
    if (const char *f = getenv("DG_FORCE_SPLITS")) fsplits = atol(f);
    // fp32 GEMMs with a short K over many rows (the Cin 3/6 layers and the
    // G.last recast: K 27..128, M >= 64K): per-layer sweep on MI355X (bs32)
    // has the 128x64 BK-16 three-blocks-per-CU tile fastest on every one
    // (D.down1 fwd 0.159 -> 0.117 ms, G.last bwd_data 0.188 -> 0.166, G.last
    // recast 0.241 -> 0.219); the MFMA-time model misses their prologue /
    // epilogue weight
    if (forced < 0 && (const TileCfg *)cfgs == kCfgs && pl.K <= 256 && pl.N <= 128 && (long)pl.M * pl.nphase >= 65536 &&
        !plan_off("shortk"))
        forced = (pl.N <= 32 && !plan_off("tile32")) ? 7 : 6;   // (32 columns: the 128 x 32 tile)
    int best = -1; double best_t = 1e30; long best_splits = 1;
    for (int c = 0; c < ncfg; ++c) {
        const TileCfg &t = cfgs[c];
        if (forced >= 0 && c != forced) continue;
        if (forced < 0 && pl.N <= 64 && t.bn > 64) continue;
        if (forced < 0 && t.bn == 32 && plan_off("tile32")) continue;
        long mt = (pl.M + t.bm - 1) / t.bm, nt = (pl.N + t.bn - 1) / t.bn;
        long tiles = mt * nt * pl.nphase;
        long ktiles = (pl.K + t.bk - 1) / t.bk;
        for (long splits = 1; splits <= std::max<long>(1, fsplits > 0 ? ktiles : ktiles / 4); splits *= 2) {
            if (fsplits > 0 && splits != fsplits) continue;
            long kt_per = (ktiles + splits - 1) / splits;
            long blocks = tiles * splits;
            long bpc = std::min<long>(t.bpc, (blocks + 255) / 256);
            double rounds = std::ceil((double)blocks / (256.0 * bpc));
            // occupancy in 4-wave units: an 8-wave block counts as two
            const long occ = std::min<long>(4, bpc * (t.wgm * t.wgn) / 4);
            double tc = rounds * bpc * 2.0 * t.bm * t.bn * kt_per * t.bk * t.eff / (cu_flops * occ_eff[occ]);
            double ts = splits > 1 ? (double)splits * pl.nphase * pl.M * pl.N * 8.0 / 5.0e12 + 2e-6 : 0.0;
            if (tc + ts < best_t) { best_t = tc + ts; best = c; best_splits = splits; }
            if (blocks >= 1024 && fsplits <= 0) break;
        }
    }
    if (best < 0) best = 0;
    pl.cfg = best;

    const TileCfg &t = cfgs[best];
    long ktiles = (pl.K + t.bk - 1) / t.bk;
    long kt_per = (ktiles + best_splits - 1) / best_splits;
    pl.kchunk = (int)(kt_per * t.bk);
    pl.splits = (int)((ktiles + kt_per - 1) / kt_per);
    pl.mtiles = (pl.M + t.bm - 1) / t.bm;
    pl.ntiles = (pl.N + t.bn - 1) / t.bn;
    return best_t;
}

// the DG_PLAN_DEBUG line of a finished plan (NARROW / NARROW_DIRECT plans, and a row-segment
// filter gradient of a narrow op, print none)
static void plan_debug(int mode, const OpPlan &pl) {
    if (!getenv("DG_PLAN_DEBUG")) return;
    switch (pl.kern) {
    case CO1: fprintf(stderr, "[dg plan] mode %d M=%d N=%d K=%d -> co1\n", mode, pl.M, pl.N, pl.K); break;
    case NTILE:
        if (!is_narrow(pl))
            fprintf(stderr, "[dg plan] mode %d M=%d N=%d K=%d -> ntile blocks %d\n", mode, pl.M, pl.N, pl.K, pl.splits);
        break;
    case SMALL:
        fprintf(stderr, "[dg plan] mode %d M=%d N=%d K=%d -> small splits %d\n", mode, pl.M, pl.N, pl.K, pl.splits);
        break;
    case NARROW_TLAST: fprintf(stderr, "[dg plan] mode %d -> tlast\n", mode); break;
    case NARROW: case NARROW_DIRECT: break;
    default:   // (GEMM, HALO_*; the cfg printed for a halo plan is its BN)
        fprintf(stderr, "[dg plan] mode %d M=%d N=%d K=%d -> %s cfg %d splits %d ph %d ptiles %d\n", mode, pl.M, pl.N, pl.K,
                kern_name(pl.kern, pl.arith), is_halo(pl.kern) ? pl.hbn : pl.cfg, pl.splits,
                is_halo(pl.kern) ? std::max(8, pl.hph) : 0, pl.ptiles);
    }
}

// step 1: the GEMM view of the op
static void gemm_view(OpPlan &pl, const ConvGeom &g, int mode) {
    if (mode == MODE_FWD) {
        pl.M = g.N * g.Ho * g.Wo; pl.N = g.Co; pl.K = g.kh * g.kw * g.Ci; pl.nphase = 1;
    } else if (mode == MODE_DGRAD) {
        pl.nphase = g.sh * g.sw;
        int Hp = (g.H + g.sh - 1) / g.sh, Wp = (g.W + g.sw - 1) / g.sw;
        pl.M = g.N * Hp * Wp; pl.N = g.Ci; pl.K = g.Th * g.Tw * g.Co;
    } else {
        pl.M = g.kh * g.kw * g.Ci; pl.N = g.Co; pl.K = g.N * g.Ho * g.Wo; pl.nphase = 1;
    }
    pl.vec = cfg_vec(g, mode, 32);
}

// step 2: the special kernels (fp32, outside the tile tables); true = pl is planned
static bool plan_special(OpPlan &pl, const ConvGeom &g, int mode, int math) {
    pl.splits = 1; pl.kchunk = pl.K;   // (a GEMM plan's choose_tiles sets its own)
    if (co1_ok(g, mode) && math != DG_MATH_FP16 && !plan_off("co1")) {
        // Co == 1 (PatchGAN last layer): direct kernels, exact fp32 FMA chains
        pl.kern = CO1;
        pl.slab_bytes = mode == MODE_WGRAD ? (size_t)co1_wgrad_blocks(g) * g.kh * g.kw * g.Ci * sizeof(float) : 0;
    } else if (mode == MODE_WGRAD && (pl.N < 8 || g.Ci < 8) && narrow_tile_ok(g) && !plan_off("ntile")) {
        // (a narrow op's filter gradient at stride 1 takes the same kernel)
        // 1-7 input channels at stride 1 (the SR discriminators' 3 -> 32 input conv): the
        // filter-gradient GEMM has Q = kh*kw*Ci <= 63 rows; the row-segment kernel instead
        pl.kern = NTILE;
        pl.splits = std::min(1024, narrow_tile_segments(g));   // partial blocks
        pl.slab_bytes = (size_t)pl.splits * pl.M * 4 * narrow_tile_groups(g) * sizeof(float);
    } else if (pl.N < 8) {   // (FWD / WGRAD: Co < 8, DGRAD: Ci < 8)
        pl.kern = NARROW;
        if (mode == MODE_WGRAD) {
            // pixels split so that taps*ci_chunks*splits ~ 1024 blocks
            long blocks = (long)g.kh * g.kw * ((g.Ci + 255) / 256);
            int s = (int)std::max<long>(1, std::min<long>(1024 / std::max<long>(blocks, 1), pl.K / 64));
            pl.splits = std::max(1, s);
            pl.kchunk = (pl.K + pl.splits - 1) / pl.splits;
            pl.slab_bytes = (size_t)pl.splits * pl.M * pl.N * sizeof(float);
        }
    } else if (small_conv_ok(g, mode, 0) && !plan_off("small")) {
        // 3 / 6 input channels, 4x4 stride 2 (G.down1, D.down1, G.last's gradients): exact fp32
        // on the 32x32x2 MFMA whatever the math mode (neither low-precision path takes Cin 3 / 6)
        pl.kern = SMALL;
        if (mode == MODE_WGRAD) {
            pl.small_rows = small_wgrad_rows_per_block(g);
            const int rows = g.N * g.Ho;
            pl.splits = (rows + pl.small_rows - 1) / pl.small_rows;
        }
        pl.slab_bytes = pl.splits > 1 ? (size_t)pl.splits * pl.M * pl.N * sizeof(float) : 0;
    } else {
        return false;
    }
    if (!is_narrow(pl)) pl.mtiles = pl.ntiles = 1;   // (a narrow op's plan leaves its tile counts 0)
    pl.ws_bytes = pl.gemm_bytes = pl.slab_bytes;
    return true;
}

// what the arithmetic choice finds and the later steps read: the operand planes' dims and
// the fp16x3 eligibility of the op
struct Elig {
    long ra, ca, rb, cb;
    bool x3_geom;   // the halo kernel's fp16x3 3x3 form applies
    bool x3_gen;    // fp16x3 on the implicit-GEMM kernel applies
    // every plane operand within the 2 GiB of a buffer resource at eb bytes per element
    bool fits(double eb) const { return eb * ra * ca < 2.0e9 && eb * rb * cb < 2.0e9; }
};

// step 3: fp32 vs bf16x6 by modelled time, then fp16, and the fp16x3 eligibility
static Elig choose_arith(OpPlan &pl, const ConvGeom &g, int mode, int math, double x6_extra) {
    // Tile + split-K choice: the cheaper of the fp32 kernel and (math mode
    // BF16X6, eligible shapes) the bf16x6 kernel plus its two split passes.
    double t32 = choose_tiles(pl, kCfgs, 157.3e12, "DG_FORCE_CFG");
    // operand planes: A is the conv input (DGRAD: the output gradient), B the filter (WGRAD: the
    // output gradient)
    const long xin = (long)g.N * g.H * g.W, xout = (long)g.N * g.Ho * g.Wo, taps_ci = (long)g.kh * g.kw * g.Ci;
    Elig e{};
    if (mode == MODE_DGRAD) { e.ra = xout; e.ca = g.Co; } else { e.ra = xin; e.ca = g.Ci; }
    e.rb = mode == MODE_WGRAD ? xout : taps_ci; e.cb = g.Co;
    bool x6_ok = g.Co % 16 == 0 && (mode == MODE_DGRAD || g.Ci % 16 == 0);
    // (the bf16x6 kernel keeps a per-row bitmask of valid taps: at most 32 taps; DG_MATH_F16X3
    // is bf16x6 wherever its fp16x3 forward does not apply)
    x6_ok = x6_ok && (math == DG_MATH_BF16X6 || math == DG_MATH_F16X3) && e.fits(6.0) && g.kh * g.kw <= 32;
    // (DG_MATH_F16X3: the halo kernel's fp16x3 form for 3x3 stride-1 forwards (Cin % 32 == 0,
    // Cout % 16 == 0, Cout > 32) and input gradients (Cout % 32 == 0 chunks the reduction over
    // output channels, Cin % 16 == 0 and Cin > 32 the BN 64 / 128 tiles), see hx3 below)
    e.x3_geom = math == DG_MATH_F16X3 && g.kh == 3 && g.kw == 3 && g.sh == 1 && g.sw == 1 &&
                !plan_off("x3") && !plan_off("halo") &&
                ((mode == MODE_FWD && g.Ci % 32 == 0 && g.Co % 16 == 0 && g.Co > 32) ||
                 (mode == MODE_DGRAD && g.Co % 32 == 0 && g.Ci % 16 == 0 && g.Ci > 32 &&
                  !plan_off("x3dgrad")));
    // fp16x3 on the implicit-GEMM kernel (conv_x6.hip NI 4) for every other eligible op of a
    // DG_MATH_F16X3 descriptor: 32-channel chunks of the activation / gradient operand,
    // 16-column weight groups
    e.x3_gen = math == DG_MATH_F16X3 && !plan_off("x3") && !plan_off("x3gen") && g.kh * g.kw <= 32 &&
               ((mode == MODE_FWD && g.Ci % 32 == 0 && g.Co % 16 == 0) ||
                (mode == MODE_DGRAD && g.Co % 32 == 0 && g.Ci % 16 == 0) ||
                (mode == MODE_WGRAD && g.Ci % 32 == 0 && g.Co % 32 == 0));
    if (x6_ok) {
        OpPlan p6 = pl;
        double t6 = choose_tiles(p6, kX6Cfgs, 2516.6e12 / 6.0, "DG_FORCE_X6CFG");
        t6 += (double)(e.ra * e.ca + e.rb * e.cb) * 10.0 / 4.0e12 + 4e-6 + x6_extra;  // split passes: read 4 B, write 6 B
        // (the implicit-GEMM fp16x3 ops where the split path beats the fp32 tiles at all: on
        // pix2pix's deepest layers (M 32..128 rows) the fp32 tiles win; DG_FORCE_X3: every
        // eligible op, for the kernel tests at small sizes.  The halo kernel's fp16x3 3x3 layers
        // stay forced: the network picks its math by image size, sr_trainer.VGGNetwork.  Plans
        // of one network in different arithmetics are safe: the host keeps weight planes per
        // layout (dg_conv_planes_format / _size), dgan/graph.py, tests/test_mixed_math_gpu.py)
        if (t6 < t32 || getenv("DG_FORCE_X6CFG") || e.x3_geom || (e.x3_gen && getenv("DG_FORCE_X3"))) {
            pl = p6;
            pl.arith = BF16X6;
        }
    }
    if (math == DG_MATH_FP16) {
        // the reference's mixed_float16 policy: one fp16 plane per operand, K-tiles of 32
        const bool ok = mode == MODE_FWD ? g.Ci % 32 == 0 && g.Co % 16 == 0
                        : (mode == MODE_DGRAD ? g.Co % 32 == 0 : g.Ci % 16 == 0 && g.Co % 16 == 0);
        if (ok && e.fits(2.0) && g.kh * g.kw <= 32) {
            choose_tiles(pl, kF16Cfgs, 2516.6e12, "DG_FORCE_F16CFG");
            pl.arith = FP16;
        }
    }
    // (an fp32 plan keeps the tiles of the first choice above)
    if (pl.arith != FP32) { pl.x6_ra = e.ra; pl.x6_ca = (int)e.ca; pl.x6_rb = e.rb; pl.x6_cb = (int)e.cb; }
    return e;
}

// step 4: the halo-tiled kernel where it applies -- 3x3 stride-1 FWD / DGRAD (kt 3), the
// sub-pixel phases of a 4x4 stride-2 DGRAD (kt 2: ConvT forwards, down-block input gradients)
// and stride-1 4x4 (kt 4) -- with its split-K / persistent-block sizing
static void plan_halo(OpPlan &pl, const ConvGeom &g, int mode, const Elig &e) {
    const bool h33 = (mode == MODE_FWD || mode == MODE_DGRAD) && g.kh == 3 && g.kw == 3 && g.sh == 1 && g.sw == 1 &&
                     pl.K % 144 == 0;
    // (phase grids that fill at least 3/4 of their 8 x 16 patches: on the deep
    // U-Net layers -- 8x8 and smaller phase grids -- the generic tiles win,
    // e.g. up3's forward 0.086 vs 0.243 ms per step)
    const int hp2 = (g.H + 1) / 2, wp2 = (g.W + 1) / 2;
    const bool h22 = mode == MODE_DGRAD && g.kh == 4 && g.kw == 4 && g.sh == 2 && g.sw == 2 && g.Th == 2 &&
                     g.Tw == 2 && pl.K % 64 == 0 &&
                     4L * hp2 * wp2 >= 3L * ((hp2 + 7) / 8 * 8) * ((wp2 + 15) / 16 * 16) && !plan_off("halo2");
    // (stride-1 4x4: the PatchGAN's 512-channel conv, input gradient only: its
    // forward measured 0.709 vs 0.668 ms on the generic 128 x 256 tiles at bs16 x2,
    // the input gradient 0.666 vs 0.690)
    const bool h44 = mode == MODE_DGRAD && g.kh == 4 && g.kw == 4 && g.sh == 1 && g.sw == 1 &&
                     pl.K % 256 == 0 && !plan_off("halo4");
    // (fp16: 3x3 only, 32-channel chunks; the forward's pool epilogue stays bf16x6)
    const bool hf16 = pl.arith == FP16 && h33 && pl.K % 288 == 0 && pl.N % 16 == 0 && !plan_off("halo_f16");
    // fp16x3 forward (DG_MATH_F16X3): 3x3 stride-1 layers with 32-channel chunks and at
    // least 48 output columns (BN 64 / 128 tiles) -- VGG19's layers after block1_conv1
    const bool hx3 = e.x3_geom && pl.arith == BF16X6 && h33 && pl.K % 288 == 0 && e.fits(4.0);
    // fp16x3 stride-2 4x4 input-gradient phases on the halo kernel (ConvT forwards, down-block
    // input gradients of G / D) where the implicit-GEMM fp16x3 plan applies (32-channel chunks)
    const bool hx3p = e.x3_gen && pl.arith == BF16X6 && h22 && pl.K % 128 == 0 && e.fits(4.0) && !plan_off("x3h2");
    // fp16x3 stride-1 4x4 (the PatchGAN's 512-channel conv, forward and input gradient) on the
    // halo kernel: 11 x 19 halo, BN 64 (72.4 KB, two blocks per CU) -- full step 982 vs 972 img/s
    // on the implicit-GEMM fp16x3 tiles (profiles/r5/ab_x3h_kt4.txt; DG_PLAN_DISABLE=x3h4)
    const bool f44 = mode == MODE_FWD && g.kh == 4 && g.kw == 4 && g.sh == 1 && g.sw == 1;
    const bool hx3q = e.x3_gen && pl.arith == BF16X6 && (h44 || f44) && pl.K % 512 == 0 && e.fits(4.0) &&
                      !plan_off("x3h4");
    if (!((pl.arith == BF16X6 && (h33 || h22 || h44 || hx3q) || hf16) && !plan_off("halo"))) return;
    // each input pixel staged once per channel chunk instead of once per tap
    pl.kern = h33 ? HALO_3x3 : (h44 || f44 ? HALO_4x4 : HALO_S2);
    const int ntap = h33 ? 9 : (h44 || f44 ? 16 : 4);
    const int bkc = (pl.arith == FP16 || hx3 || hx3p || hx3q) ? 32 : 16;   // channels per chunk
    int Hout, Wout;
    if (mode == MODE_FWD) { Hout = g.Ho; Wout = g.Wo; }
    else if (h33 || h44) { Hout = g.H; Wout = g.W; }
    else { Hout = (g.H + 1) / 2; Wout = (g.W + 1) / 2; }   // phase 0's grid, the largest
    // fp16x3 3x3 on 16 x 16 patches (8 waves, one block per CU): the K >= 4096 layers (512
    // reduction channels: VGG19 block4_conv2-4 forward and input gradient, 4-6 % faster, one
    // stream) where the grid still fills the chip at one block per CU; the shorter-K layers ran
    // 2-11 % slower on it (profiles/r6/ab_x3h_ph16.txt).  DG_X3H_PH=8|16 forces,
    // DG_PLAN_DISABLE=x3h16: 8 x 16 everywhere
    pl.hph = 8;
    if (hx3 && Hout >= 16 && pl.K >= 4096 && !plan_off("x3h16")) {
        const long t16 = (long)g.N * ((Wout + 15) / 16) * ((Hout + 15) / 16) * ((pl.N + 127) / 128);
        pl.hph = t16 >= 256 ? 16 : 8;
    }
    if (hx3)
        if (const char *ev = getenv("DG_X3H_PH")) pl.hph = atoi(ev) == 16 && Hout >= 16 ? 16 : 8;
    pl.htx = (Wout + 15) / 16;
    pl.hty = (Hout + pl.hph - 1) / pl.hph;
    // (4x4: BN 128 needs 93 KB of LDS -- one block per CU -- and measured 0.685 vs
    // 0.666 ms for BN 64, which keeps two)
    // (32 output columns, 3x3: BN 32 -- the SR family's 32-channel layers; a 64-wide tile
    // spends half its MFMAs on zero columns there)
    pl.hbn = pl.N > 64 && !h44 && !f44 ? 128 : (h33 && pl.N <= 32 && !plan_off("halo32") ? 32 : 64);
    pl.mtiles = g.N * pl.htx * pl.hty;
    // (same-box A/B of the target: 256 -0.2%, 1024 -0.8% full step vs 512)
    long target = 512;
    // (diagnostic: DG_X3_TARGET sets the fp16x3 plans' block target for same-box sweeps)
    if (hx3 && getenv("DG_X3_TARGET")) target = atol(getenv("DG_X3_TARGET"));
    // fp16x3 3x3 grids short of the target at BN 128: BN 64 tiles, twice the blocks, instead
    // of (twice the) split-K, whose partial slabs and reduce launch cost more than the halved
    // tile -- VGG19 block5 at bs32 0.148 -> 0.140 ms fwd, 0.152 -> 0.142 bwd_data, block4_conv1
    // bwd_data 0.261 -> 0.255 (profiles/r5/ab_x3h_bn64.txt; DG_PLAN_DISABLE=x3h_bn64: BN 128)
    if (pl.hph == 16) target /= 2;   // (one block per CU)
    if (hx3 && pl.hbn == 128 && (long)pl.mtiles * ((pl.N + 127) / 128) * pl.nphase < target &&
        !plan_off("x3h_bn64"))
        pl.hbn = 64;
    pl.ntiles = (pl.N + pl.hbn - 1) / pl.hbn;
    // split-K over channel chunks (at least two per split) until ~2 blocks per CU
    const long nch = pl.K / (bkc * ntap), blocks = (long)pl.mtiles * pl.ntiles * pl.nphase;
    long splits = 1;
    while (blocks * splits < target && splits * 4 <= nch) splits *= 2;
    const long cps = (nch + splits - 1) / splits;
    pl.kchunk = (int)(cps * bkc * ntap);
    pl.splits = (int)((nch + cps - 1) / cps);
    if (hx3 || hx3p || hx3q) pl.arith = F16X3;
    // fp16x3 plans with more patches than resident blocks (2 per CU): each block runs
    // several patches back to back, the next patch's halo and weights fetched under the
    // current patch's MFMAs, so a block waits for HBM once instead of once per patch.
    // ~512 blocks (one per slot) for the stride-2 phases and for 3x3 layers of <= 4
    // channel chunks per patch (VGG19 block1_conv2 fwd 0.959 -> 0.832 ms, bwd_data 1.000
    // -> 0.830, G up7 fwd 0.351 -> 0.304, down2 bwd_data 0.220 -> 0.191 at bs32); deeper
    // 3x3 layers amortise their prologue over >= 72 K-tiles and measured 1-2 % slower at
    // 512, so ~2048 there (profiles/r5/ab_x3h_persistent.txt)
    // (DG_X3H_PTILES: patches per block, DG_X3H_PDIV: the block target, for same-box A/B)
    pl.ptiles = 1;
    if (pl.arith == F16X3 && pl.splits == 1) {
        const long tot = (long)pl.mtiles * pl.ntiles * pl.nphase;
        long pdiv = hx3p || nch <= 4 ? 512 : 2048;
        if (pl.hph == 16) pdiv /= 2;   // (one block per CU)
        if (const char *ev = getenv("DG_X3H_PDIV")) pdiv = std::max(1L, atol(ev));
        long pt = tot / pdiv;
        if (const char *ev = getenv("DG_X3H_PTILES")) pt = atol(ev);
        pl.ptiles = (int)std::max(1L, std::min(pt, 64L));
    }
}

// step 5: fp16x3 on the implicit-GEMM kernel for the eligible ops the halo kernel left bf16x6
static void retile_x3(OpPlan &pl, int mode, const Elig &e) {
    if (!(e.x3_gen && pl.arith == BF16X6 && e.fits(4.0))) return;
    pl.kern = GEMM; pl.htx = pl.hty = 0;
    // short-K forward / input-gradient GEMMs (K = 16 taps x 64..128 channels: G / D down2-3
    // forwards, the up6 / up7 input gradients): the 64 x 128 tile at K 1024 and 128 x 128 at
    // K 2048 -- the MFMA-time model's 128 x 256 pick loses there to its prologue / epilogue
    // share (bs32 sweep: up7 bwd_data 0.406 -> 0.323 ms, D down2 fwd 0.238 -> 0.210, G down3
    // fwd 0.182 -> 0.167, up6 bwd_data 0.282 -> 0.263; profiles/r5/x3cfg_sweep.txt;
    // DG_PLAN_DISABLE=x3shortk: the model's pick)
    const int rule = mode == MODE_WGRAD || pl.N <= 64 || plan_off("x3shortk") ? -1
                     : (pl.K <= 1024 ? 2 : (pl.K <= 2048 ? 0 : -1));
    choose_tiles(pl, kX3Cfgs, 2516.6e12 / 3.0, "DG_FORCE_X3CFG", rule);
    pl.arith = F16X3;
}

static size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }

// step 6: workspace layout
static void layout_workspace(OpPlan &pl, const Elig &e) {
    pl.slab_bytes = pl.splits > 1 ? (size_t)pl.nphase * pl.splits * pl.M * pl.N * sizeof(float) : 0;
    pl.ws_bytes = pl.slab_bytes;
    if (reads_planes(pl.arith)) {
        // workspace: [split-K slabs][A planes][B planes] (6 B per element bf16x6, 2 B fp16, 4 B fp16x3)
        // (+ fp16x3: 8 floats for max |dy| when no scale source is set)
        const size_t eb = plane_elem_bytes(pl.arith);
        pl.x6_a_off = al256(pl.ws_bytes);
        pl.x6_b_off = al256(pl.x6_a_off + eb * e.ra * e.ca);
        pl.ws_bytes = pl.x6_b_off + eb * e.rb * e.cb;
        if (pl.arith == F16X3) {   // (max |dy| and max |x| when no scale source is set: any mode may read dy / x)
            pl.x3_max_off = al256(pl.ws_bytes);
            pl.ws_bytes = pl.x3_max_off + 2 * X3_SLOT * sizeof(float);
        }
    }
    pl.gemm_bytes = pl.ws_bytes;
}

// x6_extra: seconds the split-precision path costs beyond its GEMM and split passes (plan_all:
// a filter gradient whose operands no other op of the layer splits measures and splits both)
static OpPlan make_plan(const ConvGeom &g, int mode, int math, double x6_extra = 0.0) {
    OpPlan pl{};
    gemm_view(pl, g, mode);
    if (!plan_special(pl, g, mode, math)) {
        const Elig e = choose_arith(pl, g, mode, math, x6_extra);
        plan_halo(pl, g, mode, e);
        retile_x3(pl, mode, e);
        pl.vec = reads_planes(pl.arith) ? 1 : cfg_vec(g, mode, kCfgs[pl.cfg].bk);
        layout_workspace(pl, e);
    }
    plan_debug(mode, pl);
    return pl;
}

static ConvGeom geom_1x1(long pixels, int ci, int co) {
    ConvGeom q{};
    q.N = 1; q.H = 1; q.W = (int)pixels; q.Ci = ci; q.Ho = 1; q.Wo = (int)pixels; q.Co = co;
    q.kh = q.kw = q.sh = q.sw = 1; q.pt = q.pl = 0; q.Th = q.Tw = 1;
    return q;
}

// (a recast GEMM's operands are gathered / transposed fp32 scratch, not a layer's tensors:
// DG_MATH_F16X3 descriptors run them bf16x6)
static int recast_math(const dg_conv_desc_s *d) { return d->math == DG_MATH_F16X3 ? DG_MATH_BF16X6 : d->math; }

// decide whether a narrow op runs as a recast 1x1 MFMA GEMM (+ gather), and size its workspace
static void plan_recast(dg_conv_desc_s *d, int op) {
    Recast &rc = d->rc[op];
    rc = Recast{};
    // (a row-segment filter gradient of Co >= 8 passes here too: its Co is no recast's)
    if (!is_narrow(d->plan[op]) && d->plan[op].kern != NTILE) return;
    const ConvGeom &g = d->g;
    const int mode = engine_mode(d, op);
    const int ntap = g.kh * g.kw;
    // the 1x1 GEMM over P pixels (ci -> co channels, V rows of nvp floats after wt_floats of
    // transposed weights)
    auto gemm1 = [&](int mode1, long P, int ci, int co, int nv, int nvp, size_t wt_floats, size_t v_floats) {
        rc.nv = nv; rc.nvp = nvp; rc.mode1 = mode1;
        rc.g1 = geom_1x1(P, ci, co);
        rc.p1 = make_plan(rc.g1, mode1, recast_math(d));
        rc.v_off = al256(wt_floats * 4);
        rc.slab_off = al256(rc.v_off + v_floats * 4);
    };
    if (mode == MODE_FWD) {
        if (g.Co != 1 || g.Ci % 32 || ntap % 4 || ntap < 8) return;
        const long P = (long)g.N * g.H * g.W;
        gemm1(MODE_FWD, P, g.Ci, ntap, ntap, ntap, (size_t)g.Ci * ntap, (size_t)P * ntap);
    } else if (mode == MODE_DGRAD) {
        const int nv = ntap * g.Ci;
        // the preferred narrow kernel instead of a recast (plan_debug prints the tlast ones)
        if (tlast_ok(g) && !plan_off("tlast")) d->plan[op].kern = NARROW_TLAST;
        else if (direct_dgrad_ok(g) && !plan_off("direct")) d->plan[op].kern = NARROW_DIRECT;
        if (d->plan[op].kern != NARROW) return plan_debug(mode, d->plan[op]);
        if (g.Co % 32 || nv < 8) return;
        const int nvp = (nv + 15) & ~15;  // zero-padded columns (e.g. VGG block1_conv1: 3x3x3 = 27 -> 32)
        const long P = (long)g.N * g.Ho * g.Wo;
        gemm1(MODE_FWD, P, g.Co, nvp, nv, nvp, (size_t)g.Co * nvp, (size_t)P * nvp);
    } else {
        if (g.Co != 1 || g.Ci % 4 || g.Ci < 8 || ntap % 4) return;
        const long P = (long)g.N * g.H * g.W;
        gemm1(MODE_WGRAD, P, ntap, g.Ci, ntap, ntap, 0, (size_t)P * ntap);   // (G at offset 0, no wt)
    }
    if (is_narrow(rc.p1)) return;
    rc.bytes = rc.slab_off + rc.p1.gemm_bytes;
    rc.on = 1;
}

// workspace of run_colsum: 1024 row-chunk partials per column
static size_t colsum_ws(int C) { return (size_t)C * 1024 * sizeof(float); }

// (re)plan the three ops of a descriptor for its math mode
void plan_all(dg_conv_desc_s *d) {
    for (int op = 0; op < 3; ++op) {
        // (DG_MATH_F16X3: fp16x3 wherever make_plan finds the op eligible, bf16x6 elsewhere)
        // A filter gradient reads the layer's input and output gradient, whose fp16x3 planes exist
        // only where the forward / input gradient of the layer runs fp16x3 (the producers write
        // them for those ops); otherwise its split path also zeroes a max slot and measures the
        // operand (memset + absmax launches and a read) before splitting it -- G down7 / up2
        // filter gradients: 37 us of passes around a 27-42 us GEMM (round 6, profiles/r6/calls.txt)
        double extra = 0.0;
        if (op == DG_OP_BWD_FILTER && d->math == DG_MATH_F16X3) {
            const double xin = (double)d->N * d->H * d->W * d->Cin, gout = (double)d->N * d->Ho * d->Wo * d->Cout;
            if (d->plan[DG_OP_FWD].arith != F16X3) extra += 8e-6 + xin * 4.0 / 4.0e12;
            if (d->plan[DG_OP_BWD_DATA].arith != F16X3) extra += 8e-6 + gout * 4.0 / 4.0e12;
        }
        d->plan[op] = make_plan(d->g, engine_mode(d, op), d->math, plan_off("wgrad_extra") ? 0.0 : extra);
        plan_recast(d, op);
        if (d->rc[op].on) d->plan[op].ws_bytes = d->rc[op].bytes;
        if (op == DG_OP_BWD_FILTER) {
            // room for the bias column sum partials after the split-K slabs
            size_t base = d->rc[op].on ? d->rc[op].bytes : d->plan[op].gemm_bytes;
            d->plan[op].colsum_off = al256(base);
            d->plan[op].ws_bytes = d->plan[op].colsum_off + colsum_ws(d->Cout);
        }
    }
}

int default_math() {
    const char *m = getenv("DG_CONV_MATH");
    if (m && (!strcmp(m, "fp32") || !strcmp(m, "0"))) return DG_MATH_FP32;
    if (m && (!strcmp(m, "fp16") || !strcmp(m, "2"))) return DG_MATH_FP16;
    if (m && (!strcmp(m, "f16x3") || !strcmp(m, "3"))) return DG_MATH_F16X3;
    return DG_MATH_BF16X6;
}

// the forward plan of d can run MaxPool2D(2) in its epilogue: the halo-tiled
// bf16x6 kernel with one split over whole 8 x 16 patches, and an activation
// whose derivative is a function of the output's sign
bool pool_fusable(const dg_conv_desc_s *d, int act) {
    const OpPlan &pl = d->plan[DG_OP_FWD];
    return !d->transpose && (pl.arith == BF16X6 || pl.arith == F16X3) && pl.kern == HALO_3x3 && pl.hbn != 32 &&
           pl.splits == 1 && !d->rc[DG_OP_FWD].on &&
           d->g.Ho % (pl.hph == 16 ? 16 : 8) == 0 &&
           d->g.Wo % 16 == 0 && d->g.Co % 16 == 0 &&
           (act == DG_ACT_NONE || act == DG_ACT_RELU || act == DG_ACT_LRELU);
}

// layer tensors (DG_TENSOR_*) read as engine operands A and B by op
void op_tensors(const dg_conv_desc_s *d, int op, int &ta, int &tb) {
    if (op == DG_OP_FWD) { ta = DG_TENSOR_X; tb = DG_TENSOR_W; }
    else if (op == DG_OP_BWD_DATA) { ta = DG_TENSOR_DY; tb = DG_TENSOR_W; }
    else if (!d->transpose) { ta = DG_TENSOR_X; tb = DG_TENSOR_DY; }
    else { ta = DG_TENSOR_DY; tb = DG_TENSOR_X; }  // conv view of a transposed layer: A = its output grad
}

// an op that reads operand planes at all: bf16x6, the fp16 copy (DG_MATH_FP16: [rows][C]
// fp16, the same for every op that reads the tensor) or fp16x3; fp32 / narrow / recast
// plans read fp32
static bool op_reads_planes(const dg_conv_desc_s *d, int op) {
    const OpPlan &pl = d->plan[op];
    if (!reads_planes(pl.arith) || d->rc[op].on || pl.M == 0 || pl.N == 0) return false;
    return !(pl.arith == FP16 && plan_off("f16planes"));
}
// tensor t's planes are fp16x3 when an fp16x3 op reads them; a bf16x6 op of the same
// layer then splits that tensor itself, except w, whose buffer holds [fp16x3 | bf16x6]
bool tensor_reader(const dg_conv_desc_s *d, int t, Arith arith) {
    for (int op = 0; op < 3; ++op) {
        int ta, tb;
        op_tensors(d, op, ta, tb);
        if (((ta | tb) & t) && op_reads_planes(d, op) && d->plan[op].arith == arith) return true;
    }
    return false;
}
size_t x3_wbytes(const dg_conv_desc_s *d) {
    return al256((size_t)4 * d->g.kh * d->g.kw * d->Cin * d->Cout);
}
size_t tensor_plane_bytes(const dg_conv_desc_s *d, int t) {
    const size_t nw = (size_t)d->g.kh * d->g.kw * d->Cin * d->Cout;
    if (t == DG_TENSOR_X) return (size_t)(tensor_x3(d, t) ? 4 : 6) * d->N * d->H * d->W * d->Cin;
    if (t == DG_TENSOR_DY) return (size_t)(tensor_x3(d, t) ? 4 : 6) * d->N * d->Ho * d->Wo * d->Cout;
    if (!tensor_x3(d, t)) return 6 * nw;
    return x3_wbytes(d) + (tensor_reader(d, t, BF16X6) ? 6 * nw : 0);
}

// tensors op reads as operand planes (op_reads_planes); x and dy only in the format
// tensor_x3 gives them
int op_plane_mask(const dg_conv_desc_s *d, int op) {
    if (!op_reads_planes(d, op)) return 0;
    int ta, tb;
    op_tensors(d, op, ta, tb);
    const bool x3 = d->plan[op].arith == F16X3;
    int m = ta | tb;
    for (int t : {DG_TENSOR_X, DG_TENSOR_DY})
        if ((m & t) && tensor_x3(d, t) != x3) m &= ~t;
    return m;
}

}  // namespace dg
