// Tile configurations of the implicit-GEMM conv kernels, written once: the planner's cost
// tables (conv_plan.hip) and the launch switches (conv.hip launch_gemm, conv_x6.hip
// launch_gemm_planes / launch_gemm_x3) are both generated from these lists, so the index of a
// planner row is the case that launches it.
//
// Columns: X(index, BM, BN, WGM, WGN, BK, MINW, NBUF, bpc, eff)
//   BM x BN   block tile
//   WGM x WGN wave grid
//   BK        K-tile depth
//   MINW      min waves/SIMD the kernel is compiled for (register budget)
//   NBUF      LDS buffers of the K pipeline (the fp32 kernel has one form: 1)
//   bpc       resident blocks per CU (LDS / registers), for the planner's occupancy model
//   eff       relative cost per FLOP (measured on MI355X), for the planner
#pragma once

// fp32 MFMA kernel (conv.hip k_conv_gemm)
// (7, 8: 32-wide tiles for the 32-channel layers of the SR discriminators (srgan.py:232-272):
// a 64-wide tile computes half zeros there)
#define DG_TILES_FP32(X)                                                                         \
    X(0, 128, 128, 2, 2, 32, 2, 1, 2, 1.00)                                                      \
    X(1, 128, 64, 2, 2, 32, 2, 1, 2, 1.12)                                                       \
    X(2, 64, 128, 2, 2, 32, 2, 1, 2, 1.12)                                                       \
    X(3, 64, 64, 2, 2, 32, 2, 1, 3, 1.35)                                                        \
    X(4, 32, 128, 1, 4, 32, 2, 1, 3, 1.50)                                                       \
    X(5, 128, 128, 2, 2, 16, 3, 1, 3, 1.00)                                                      \
    X(6, 128, 64, 2, 2, 16, 3, 1, 3, 1.12)                                                       \
    X(7, 128, 32, 4, 1, 32, 2, 1, 3, 1.40)                                                       \
    X(8, 256, 32, 4, 1, 32, 2, 1, 2, 1.30)

// bf16x6 and fp16 kernels (conv_x6.hip k_conv_gemm_x6, NI 3 / 2): the same tiles; BK here is
// the bf16x6 K-tile, the fp16 kernel's is DG_TILES_F16_BK
// (6: 32-wide, SR discriminators' 32-channel layers)
#define DG_TILES_F16_BK 32
#define DG_TILES_X6(X)                                                                           \
    X(0, 128, 128, 2, 2, 16, 2, 3, 2, 1.00)                                                      \
    X(1, 128, 64, 2, 2, 16, 2, 3, 2, 1.15)                                                       \
    X(2, 64, 128, 2, 2, 16, 2, 3, 2, 1.15)                                                       \
    X(3, 64, 64, 2, 2, 16, 3, 3, 4, 1.40)                                                        \
    X(4, 256, 128, 4, 2, 16, 2, 3, 1, 1.00)                                                      \
    X(5, 128, 256, 2, 4, 16, 2, 3, 1, 0.90)                                                      \
    X(6, 128, 32, 4, 1, 16, 3, 3, 4, 1.45)

// fp16x3 kernel (conv_x6.hip k_conv_gemm_x6, NI 4): four 16-wide images per K-tile of 32, so
// the 128-wide tiles keep one K-tile ahead in two LDS buffers (67 KB at 128 x 128: two blocks
// per CU), the narrow ones two ahead in three.  The 8-wave tiles (4, 5) run the two-half K loop
// (conv_x6.hip ktile_w8), which needs a third buffer: a tile's buffer lives until the later
// half has read it (149,760 B at 128 x 256, one block per CU either way); DG_X3_W8_LOCKSTEP
// builds the lock-step loop on two buffers for A/B runs.  Their eff values are those fitted on
// the lock-step loop: the two-half loop runs the filter gradients 21 % faster (profiles/w8), but
// a lower eff would move plans of tests/plan_snapshot.json, so the planner keeps the old cost
#ifndef DG_X3_NB45
#ifdef DG_X3_W8_LOCKSTEP
#define DG_X3_NB45 2
#else
#define DG_X3_NB45 3
#endif
#endif
#ifndef DG_X3_NB0
#define DG_X3_NB0 2
#endif
#ifndef DG_X3_NB12
#define DG_X3_NB12 2
#endif
#define DG_TILES_X3(X)                                                                           \
    X(0, 128, 128, 2, 2, 32, 2, DG_X3_NB0, 2, 1.00)                                              \
    X(1, 128, 64, 2, 2, 32, 2, DG_X3_NB12, 3, 1.15)                                              \
    X(2, 64, 128, 2, 2, 32, 2, DG_X3_NB12, 3, 1.15)                                              \
    X(3, 64, 64, 2, 2, 32, 3, 3, 3, 1.40)                                                        \
    X(4, 256, 128, 4, 2, 32, 1, DG_X3_NB45, 1, 1.00)                                             \
    X(5, 128, 256, 2, 4, 32, 1, DG_X3_NB45, 1, 0.90)                                             \
    X(6, 128, 32, 4, 1, 32, 3, 3, 2, 1.45)
