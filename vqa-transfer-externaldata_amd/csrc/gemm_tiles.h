// The tile configurations of gemm_f32_kernel (gemm_f32.hip), each written down once, and the four id namespaces that
// name them: plain ids (vqa_gemm_set_config, choose(), the VQA_HOT_*_CFG overrides), GRU-step ids
// (vqa_gemm_set_gru_config, VQA_HOT_GRU_*), conv ids (vqa_conv_set_config) and tall ids (vqa_gemm_set_tall_config).
// Every dispatcher of gemm_f32.hip names an entry of VQA_GEMM_TILES; none repeats a tile's numbers.  To add a tile: one
// row here (a PLAIN row takes the next id), one row in tests/gemm_ref.py::CFG, and a row in whichever id table below
// should reach it.  Internal: gemm_f32.hip includes it (and gru_step.hip, for the ids that are no tile), other translation units ask through
// gemm_args.h.
#pragma once
#include "vqa_common.h"

// BM x BN workgroup tile of WM x WN wave tiles (32x32 MFMA tiles), WGK in-block k groups, BK-deep k tiles, DEEP = two
// tiles of register prefetch instead of one, NT threads = (BM / WM) (BN / WN) WGK waves
template <int BM_, int BN_, int WM_, int WN_, int WGK_, int BK_, bool DEEP_, int NT_>
struct Tile {
    static constexpr int BM = BM_, BN = BN_, WM = WM_, WN = WN_, WGK = WGK_, BK = BK_, NT = NT_;
    static constexpr bool DEEP = DEEP_;
};

// PLAIN(plain id, BM, BN, WM, WN, WGK, BK, DEEP, NT); GRU_ONLY(name, the same eight): a tile that only the fused
// GRU-step kernels take.  Plain ids are part of the C ABI (vqa_gemm_set_config) and of the tuning files under
// profiles/: rows keep their ids.
#define VQA_GEMM_TILES(PLAIN, GRU_ONLY)                                                                                 \
    PLAIN(0, 128, 128, 64, 64, 1, 16, false, 256)                                                                       \
    PLAIN(1, 128, 128, 64, 64, 1, 32, false, 256)                                                                       \
    PLAIN(2, 64, 64, 32, 32, 1, 16, false, 256)                                                                         \
    PLAIN(3, 64, 64, 32, 32, 1, 32, false, 256)                                                                         \
    PLAIN(4, 64, 64, 32, 32, 1, 64, false, 256)                                                                         \
    PLAIN(5, 128, 64, 64, 32, 1, 32, false, 256)                                                                        \
    PLAIN(6, 64, 128, 32, 64, 1, 32, false, 256)                                                                        \
    PLAIN(7, 64, 32, 32, 32, 2, 64, false, 256)                                                                         \
    PLAIN(8, 32, 32, 32, 32, 4, 64, false, 256)                                                                         \
    PLAIN(9, 32, 64, 32, 32, 2, 64, false, 256)                                                                         \
    PLAIN(10, 64, 64, 32, 32, 1, 64, true, 256)                                                                         \
    PLAIN(11, 64, 32, 32, 32, 2, 64, true, 256)                                                                         \
    PLAIN(12, 64, 64, 32, 32, 1, 32, true, 256)                                                                         \
    PLAIN(13, 64, 32, 32, 32, 2, 32, true, 256)                                                                         \
    PLAIN(14, 128, 32, 32, 32, 1, 64, true, 256)                                                                        \
    PLAIN(15, 128, 64, 32, 64, 1, 32, true, 256)                                                                        \
    PLAIN(16, 128, 128, 64, 32, 1, 32, false, 512)                                                                      \
    PLAIN(17, 128, 128, 32, 64, 1, 32, false, 512)                                                                      \
    PLAIN(18, 256, 64, 64, 32, 1, 32, false, 512)                                                                       \
    PLAIN(19, 128, 128, 64, 32, 1, 16, false, 512)                                                                      \
    PLAIN(20, 128, 64, 32, 32, 1, 32, false, 512)                                                                       \
    PLAIN(21, 64, 128, 32, 32, 1, 32, false, 512)                                                                       \
    PLAIN(22, 128, 64, 32, 32, 1, 16, false, 512)                                                                       \
    PLAIN(23, 64, 32, 32, 32, 4, 32, true, 512)                                                                         \
    GRU_ONLY(Gru32x32, 32, 32, 32, 32, 4, 32, true, 256)                                                                \
    GRU_ONLY(Gru1024Gates, 64, 64, 32, 32, 4, 64, true, 1024)                                                           \
    GRU_ONLY(Gru1024Narrow, 64, 32, 32, 32, 8, 64, true, 1024)

template <int ID> struct PlainTile;                               // PlainTile<id>::type = the tile of plain id `id`
#define VQA_TILE_PLAIN(ID, ...) template <> struct PlainTile<ID> { using type = Tile<__VA_ARGS__>; };
#define VQA_TILE_GRU_ONLY(NAME, ...) using NAME = Tile<__VA_ARGS__>;
VQA_GEMM_TILES(VQA_TILE_PLAIN, VQA_TILE_GRU_ONLY)
#undef VQA_TILE_PLAIN
#undef VQA_TILE_GRU_ONLY
template <int ID> using Plain = typename PlainTile<ID>::type;
#define VQA_TILE_NONE(...)

// what choose() needs of a plain id at run time: tile counts and the split
struct PlainDims { int id, BM, BN; };
#define VQA_TILE_DIMS(ID, BM, BN, ...) {ID, BM, BN},
constexpr PlainDims kPlainDims[] = {VQA_GEMM_TILES(VQA_TILE_DIMS, VQA_TILE_NONE)};
#undef VQA_TILE_DIMS
constexpr int NUM_CFG = sizeof(kPlainDims) / sizeof(kPlainDims[0]);
constexpr bool plain_ids_are_row_numbers() {
    for (int i = 0; i < NUM_CFG; ++i)
        if (kPlainDims[i].id != i) return false;
    return true;
}
static_assert(plain_ids_are_row_numbers(), "kPlainDims is indexed by plain id");

// the one test of a plain id, whoever it came from (a setter, the environment)
inline bool is_plain_cfg(int id) { return id >= 0 && id < NUM_CFG; }

// fn(Plain<id>{}) for a plain id; VQA_ERR_ARG for any other value
template <typename F>
inline int with_plain_tile(int id, F&& fn) {
    switch (id) {
#define VQA_TILE_CASE(ID, ...) case ID: return fn(Plain<ID>{});
        VQA_GEMM_TILES(VQA_TILE_CASE, VQA_TILE_NONE)
#undef VQA_TILE_CASE
        default: return VQA_ERR_ARG;
    }
}
#undef VQA_TILE_NONE

// Ragged / unaligned shapes, whatever id was asked for: the guarded loaders (EDGE) on the smallest 4-wave tile
using EdgeTile = Plain<2>;

// GRU-step ids: X(id, tile of the 2H-wide gate GEMM (EPI_GATES), tile of the H-wide GEMMs (the other three epilogues)).
// The numbering is this table's own: 16 and 17 are not plain 16 and 17.  Id 18 is one 16-wave workgroup per CU, 64x64
// tiles for the gate GEMM and 64x32 for the others.
#define VQA_GRU_CFGS(X)                  \
    X(4, Plain<4>, Plain<4>)             \
    X(7, Plain<7>, Plain<7>)             \
    X(8, Plain<8>, Plain<8>)             \
    X(9, Plain<9>, Plain<9>)             \
    X(10, Plain<10>, Plain<10>)          \
    X(11, Plain<11>, Plain<11>)          \
    X(12, Plain<12>, Plain<12>)          \
    X(13, Plain<13>, Plain<13>)          \
    X(16, Gru32x32, Gru32x32)            \
    X(17, Plain<23>, Plain<23>)          \
    X(18, Gru1024Gates, Gru1024Narrow)   \
    X(20, Plain<20>, Plain<20>)          \
    X(21, Plain<21>, Plain<21>)
// ... and one id that is no tile: the register-streamed step kernels (vqa_gru_rs_launch, gru_stream.hip); the shapes
// they do not take run under the fallback id
constexpr int GRU_CFG_STREAMED = 30;
constexpr int GRU_CFG_STREAMED_FALLBACK = 16;
// ... and one that is no tile of gemm_f32_kernel at all: the per-step drivers (gru_step.hip) run their step GEMMs on the
// bf16 matrix unit (gru_step_bf16.hip).  vqa_gemm_set_gru_config admits it; vqa_gru_step_launch never sees it.
constexpr int GRU_CFG_BF16 = 64;

// conv ids of the implicit-GEMM convolutions: X(conv id, plain id of its tile).  (The 1x1 path names plain ids itself.)
#define VQA_CONV_CFGS(X) X(0, 3) X(1, 20) X(2, 21) X(3, 16)
#define VQA_TILE_COUNT(...) +1
constexpr int NUM_CONV_CFG = 0 VQA_CONV_CFGS(VQA_TILE_COUNT);
#undef VQA_TILE_COUNT

// tall ids: the plain ids that choose() may give tall activations x wide weights (g_tall_cfg), and so the tiles of the
// row-gathered product, which takes g_tall_cfg's: X(plain id)
#define VQA_TALL_CFGS(X) X(20) X(21)
