// Host side of the conv engine: what a layer op's plan is (OpPlan: kernel, arithmetic, tile,
// split-K, workspace layout), the descriptor that holds the three plans of a layer, and the
// planner's entry points (conv_plan.hip).  conv.hip launches what is planned here.
#pragma once
#include "conv_impl.h"

namespace dg {

// tile config of an implicit-GEMM kernel (conv_tiles.h): block tile, wave grid, K-tile depth,
// resident blocks per CU (LDS / registers), relative cost per FLOP (measured on MI355X)
struct TileCfg {
    int bm, bn, wgm, wgn, bk, bpc;
    double eff;
};

// arithmetic of an op's GEMM: the values dg_conv_op_arith returns
enum Arith : int { FP32 = DG_MATH_FP32, BF16X6 = DG_MATH_BF16X6, FP16 = DG_MATH_FP16, F16X3 = DG_MATH_F16X3 };
static_assert(FP32 == DG_MATH_FP32 && BF16X6 == DG_MATH_BF16X6 && FP16 == DG_MATH_FP16 && F16X3 == DG_MATH_F16X3,
              "Arith is DG_MATH_*");
static_assert(FP32 == 0, "a zeroed OpPlan is an fp32 plan");

// kernel family of an op
enum Kern {
    GEMM = 0,       // implicit GEMM on the arithmetic's tile table (cfg)
    HALO_3x3,       // halo-tiled kernel (conv_x6h.hip): stride-1 3x3 FWD / DGRAD
    HALO_S2,        //   the sub-pixel phases of a stride-2 4x4 DGRAD
    HALO_4x4,       //   stride-1 4x4
    NARROW,         // VALU narrow kernels (GEMM N < 8), or the op's recast (Recast)
    NARROW_DIRECT,  //   narrow DGRAD, k_direct_dgrad preferred (dy halo staged in LDS)
    NARROW_TLAST,   //   narrow DGRAD, the fused MFMA + col2im kernel preferred (conv_tlast.hip)
    NTILE,          // narrow stride-1 filter gradient on row segments (k_narrow_wgrad_tile)
    SMALL,          // small-Cin strip kernels (conv_small.hip)
    CO1,            // single-output-channel direct kernels (conv_co1.hip)
};
// (NARROW_DIRECT / NARROW_TLAST name a preference: run_engine falls back to k_narrow_dgrad when
// a mask is present or the operands are misaligned)

inline bool is_halo(Kern k) { return k == HALO_3x3 || k == HALO_S2 || k == HALO_4x4; }
// taps per axis the halo kernel is instantiated for (launch_gemm_x6h's kt)
inline int halo_taps(Kern k) { return k == HALO_S2 ? 2 : (k == HALO_4x4 ? 4 : 3); }
// the arithmetics whose kernels read operand planes instead of fp32
inline bool reads_planes(Arith a) { return a != FP32; }
// bytes per element of an operand's planes: bf16 hi/mid/lo 6, one fp16 2, fp16 h + l 4
inline int plane_elem_bytes(Arith a) { return a == FP16 ? 2 : (a == F16X3 ? 4 : 6); }
// the name DG_PLAN_DEBUG prints for a GEMM / halo plan (tests/test_plan.py, tests/test_x3_gpu.py
// and scripts/diag/x3_cfg_check.py parse it; fp16x3 4x4 halo plans print x6h4 like the bf16x6 ones)
inline const char *kern_name(Kern k, Arith a) {
    switch (k) {
    case HALO_S2: return a == F16X3 ? "x3h2" : "x6h2";
    case HALO_4x4: return "x6h4";
    case HALO_3x3: return a == FP16 ? "f16h" : (a == F16X3 ? "x3h" : "x6h");
    default: return a == FP16 ? "f16" : (a == F16X3 ? "x3" : (a == BF16X6 ? "x6" : "fp32"));
    }
}

struct OpPlan {
    Kern kern;
    Arith arith;     // of a GEMM / HALO_* plan (the other kernels are fp32): BF16X6 the split-precision
                     // kernel, FP16 one fp16 plane per operand, F16X3 (DG_MATH_F16X3), else fp32 MFMA
    int cfg;         // tile config index in the arithmetic's table (conv_tiles.h)
    int vec;
    int splits, kchunk;
    int M, N, K, nphase;
    int mtiles, ntiles;
    size_t slab_bytes;  // split-K partial slabs
    size_t gemm_bytes;  // workspace of the GEMM (split-K slabs + bf16x6 planes)
    size_t ws_bytes;    // total workspace of the layer op (GEMM + bias partials)
    size_t colsum_off;  // bwd_filter: offset of the bias column-sum partials
    // operand planes: dims (rows x C for A and B) and workspace offsets
    long x6_ra, x6_rb;
    int x6_ca, x6_cb;
    size_t x6_a_off, x6_b_off;
    // halo-tiled kernel (HALO_*): its BN, tiles of hph x 16 output pixels
    // (hph 8, or 16: the fp16x3 3x3 16 x 16 patch on 8 waves)
    int hbn, htx, hty, hph;
    // fp16x3 halo plans without split-K: patches per block (persistent blocks, conv_x6h.hip)
    int ptiles;
    // SMALL WGRAD: conv-view output rows per block
    int small_rows;
    // fp16x3 input gradient: workspace offset of the max |dy| float (no scale source set)
    size_t x3_max_off;   // (+X3_SLOT floats: max |x| when the x operand has no scale source)
};
// a narrow op (GEMM N < 8, no Co-1 kernel): the VALU narrow kernels, or its row-segment filter gradient
inline bool is_narrow(const OpPlan &pl) {
    return pl.kern == NARROW || pl.kern == NARROW_DIRECT || pl.kern == NARROW_TLAST || (pl.kern == NTILE && pl.N < 8);
}

// A narrow op (GEMM N <= 8) recast as a 1x1-geometry MFMA GEMM plus a gather:
//   FWD,   Co == 1 : V[p_in][(i,j)]      = x[p_in][:] . w[(i,j)][:]   ; y = shift-and-add of V
//   DGRAD, Ci <= 8 : V[p_out][(i,j,ci)]  = dy[p_out][:] . w[(i,j,ci)][:] ; dx = col2im(V)
//   WGRAD, Co == 1 : dw[(i,j)][ci]       = sum_p G[p][(i,j)] x[p][ci], G = dy gathered per tap
struct Recast {
    int on;
    int mode1;          // engine mode of the 1x1 GEMM
    ConvGeom g1;        // its geometry (N=1, H=1, W=pixels)
    OpPlan p1;          // its plan
    int nv;             // columns of V / G
    int nvp;            // row stride of V (nv rounded up so the 1x1 GEMM stays on the bf16x6 path)
    size_t wt_off, v_off, slab_off, bytes;
};

}  // namespace dg

struct dg_conv_desc_s {
    int transpose;
    int math;                        // DG_MATH_*
    // fp16x3 input gradient scale context (dg_conv_set_grad_scale): sources (m, g) of the dy
    // and dx planes' scales, and where max |dx| goes (device pointers; NULL = unset)
    const float *gs_dy_m, *gs_dy_g, *gs_dx_m, *gs_dx_g;
    float *gs_dx_max;
    // fp16x3 activation scale context (dg_conv_set_act_scale): source (m, g, c) of the x planes'
    // scale, of the forward's output planes' scale, and where max |y| of the forward goes
    const float *as_x_m, *as_x_g, *as_x_c, *as_y_m, *as_y_g, *as_y_c;
    float *as_y_max;
    int N, H, W, Cin, Cout, Ho, Wo;  // layer view
    dg::ConvGeom g;                  // conv view
    dg::OpPlan plan[3];              // indexed by DG_OP_*
    dg::Recast rc[3];
};

namespace dg {

// caller-held bf16x6 planes of the two engine operands (dg_conv_planes_t mapped
// onto A / B of one op): NULL = split into the workspace; ready = already split
struct PlaneRefs {
    void *a, *b;
    int a_ready, b_ready;
    size_t b_x6;   // (fp16x3 op, B = w) the weight buffer also holds bf16x6 planes, b_x6 bytes in (0: none)
};

// Host geometry predicates of the VALU kernels in conv.hip that both the planner and a launch use
// (beside small_conv_ok, co1_ok and tlast_ok of conv_impl.h).
// k_direct_dgrad's tile: 8 x 32 phase pixels, 32-channel chunks (pixel stride 36 floats in LDS)
constexpr int DIR_PH = 8, DIR_PW = 32, DIR_CC = 32, DIR_CS = DIR_CC + 4;
// direct DGRAD kernels instantiated: (Ci, taps per phase) of the layers above
// (measured per layer in the training step: VGG block1_conv1 dgrad 0.210 ->
// 0.172 ms (0.132 with the batched, prefetched halo loads), D.down1 dgrad
// 0.208 -> 0.122 ms; G.last forward with Co 128 ran 0.239 -> 0.38 ms, so
// Co > 64 stays on the GEMM recast)
inline bool direct_dgrad_ok(const ConvGeom &g) {
    if (g.Co % DIR_CC || g.Co > 64) return false;
    const bool t33 = g.Th == 3 && g.Tw == 3, t22 = g.Th == 2 && g.Tw == 2;
    return (g.Ci == 3 && (t33 || t22)) || (g.Ci == 6 && t22);
}
// k_narrow_wgrad_tile: row segments of NWT_TP pixels
constexpr int NWT_TP = 64;
constexpr int NWT_QMAX = 4;    // slots per thread: Q * CG <= 1024
inline int narrow_tile_groups(const ConvGeom &g) { return (g.Co + 3) / 4; }
inline size_t narrow_tile_lds(const ConvGeom &g) {
    return ((size_t)g.kh * (NWT_TP + g.kw - 1) * g.Ci + 4 * NWT_TP * (size_t)narrow_tile_groups(g)) * sizeof(float);
}
inline bool narrow_tile_ok(const ConvGeom &g) {
    const long S = (long)g.kh * g.kw * g.Ci * narrow_tile_groups(g);
    return g.sh == 1 && g.sw == 1 && S <= 256L * NWT_QMAX && narrow_tile_lds(g) <= 64 * 1024;
}
inline int narrow_tile_segments(const ConvGeom &g) {
    return g.N * g.Ho * ((g.Wo + NWT_TP - 1) / NWT_TP);
}

// layer op -> conv-view engine (MODE_*)
int engine_mode(const dg_conv_desc_s *d, int op);
// DG_PLAN_DISABLE holds feature
bool plan_off(const char *feature);
int default_math();
// (re)plan the three ops of a descriptor for its math mode
void plan_all(dg_conv_desc_s *d);
// the forward plan of d can run MaxPool2D(2) in its epilogue
bool pool_fusable(const dg_conv_desc_s *d, int act);

// plane ownership: which layer tensors (DG_TENSOR_*) an op reads as operand planes, in which
// format, and how large a caller-held plane buffer is
void op_tensors(const dg_conv_desc_s *d, int op, int &ta, int &tb);
bool tensor_reader(const dg_conv_desc_s *d, int t, Arith arith);
inline bool tensor_x3(const dg_conv_desc_s *d, int t) { return tensor_reader(d, t, F16X3); }
size_t x3_wbytes(const dg_conv_desc_s *d);
size_t tensor_plane_bytes(const dg_conv_desc_s *d, int t);
int op_plane_mask(const dg_conv_desc_s *d, int op);

}  // namespace dg
