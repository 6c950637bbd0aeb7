// gz_pvnet.h -- packed weight layout of AlphaZeroGomokuNet (neural_network.py:94-159)
// for the fp32 MFMA forward.  Produced by gzero/weights.py:pack_pv_weights().
//
// Conv weights are stored K-major as the GEMM B operand W[k][n]:
//   conv0:     k = tap*3 + cin   (27 rows + 1 zero row), n = out channel (128)
//   res convs: k = tap*128 + cin (1152 rows),           n = out channel (128)
// with tap = kh*3 + kw.  Bias and eval-mode BatchNorm are folded into a
// per-channel affine epilogue: y = acc*S[n] + T[n],
//   S = gamma / sqrt(running_var + eps), T = (bias - running_mean)*S + beta.
// Head weights: 1x1 convs as [out][128]; FCs stored transposed ([in][out]) so a
// thread per output reads coalesced rows.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>

namespace gzpv {
constexpr int CH = 128;
constexpr int POS = 225;
constexpr int K0 = 28;          // 27 padded to a multiple of the MFMA K-step (2)
constexpr int K = 9 * CH;       // 1152

constexpr int C0_W = 0;
constexpr int C0_S = C0_W + K0 * CH;
constexpr int C0_T = C0_S + CH;
constexpr int RES0 = C0_T + CH;
constexpr int RES_STRIDE = K * CH + 2 * CH;  // W, S, T
constexpr int RES_W = 0, RES_S = K * CH, RES_T = K * CH + CH;
constexpr int P_W = RES0 + 4 * RES_STRIDE;   // [2][128]
constexpr int P_B = P_W + 2 * CH;            // [2] (+2 pad)
constexpr int PF_WT = P_B + 4;               // [450][225]
constexpr int PF_B = PF_WT + 450 * 225;      // [225] (+3 pad)
constexpr int V_W = PF_B + 228;              // [128]
constexpr int V_B = V_W + CH;                // [1] (+3 pad)
constexpr int V1_WT = V_B + 4;               // [225][64]
constexpr int V1_B = V1_WT + 225 * 64;       // [64]
constexpr int V2_W = V1_B + 64;              // [64]
constexpr int V2_B = V2_W + 64;              // [1] (+3 pad)
// fp16x3 section: per residual conv, fp16 hi then fp16 lo (2 halves per float
// slot), each in v_mfma_f32_16x16x32_f16 B-fragment order
//   [ks 36][n-tile 8][lane 64][8]:  n = 16*n_tile + lane%16, k = 32*ks + 8*(lane/16) + j
// so one wave's fragment is one contiguous 1 KiB load; S/T are shared with the fp32 section
constexpr int F16_RES0 = (V2_B + 4 + 3) & ~3;  // 16-byte aligned for h8 loads
constexpr int F16_STRIDE = K * CH;           // floats: K*CH halves hi + K*CH halves lo
// conv0 in fp16 MFMA A-fragment order [n-tile 8][lane 64][8]: n = 16*n_tile + lane%16,
// k = 8*(lane/16) + j (k >= 27 zero); hi then lo
constexpr int F16_C0 = F16_RES0 + 4 * F16_STRIDE;
// FC heads in MFMA B-fragment order for the batched heads kernel (gz_f16conv.h
// heads_gemm_block): policy_fc [29 k-blocks][15 n-tiles][64][4], value_fc1 [15][4][64][4]
constexpr int PF_P = F16_C0 + 8 * 64 * 8;
constexpr int PF_KB = 29, PF_NT = 15;
constexpr int V1_P = PF_P + PF_KB * PF_NT * 256;
constexpr int V1_KB = 15, V1_NT = 4;
constexpr int TOTAL = V1_P + V1_KB * V1_NT * 256;

// incremental forward (gz_pvinc.hip): a root board's intermediate maps x0, y1, x1,
// y2 are stored in the LDS layout of the f16x3 kernel: hi plane [16 ch-groups]
// [256 rows][8] then the lo plane -- PV_MAP_HALVES halves per map
constexpr int PV_MAP_PLANE = CH * 256;
constexpr int PV_MAP_HALVES = 2 * PV_MAP_PLANE;
// delta tree forward (gz_pvdg.hip, pv_dg_kernel): a root board's pre-ReLU values
// of the 4 residual layers (y1, x1, y2, x2: z = BN(conv) [+ skip input]), fp32
// position-major [256 positions][128 channels] -- PV_PRE_FLOATS floats per layer
constexpr int PV_PRE_FLOATS = 256 * CH;
// a root child's patch (written when it has children of its own, read by their delta
// pass): fp32, position-major [position][128 channels] -- its x0 (post-ReLU) in the
// radius-1 square around its stone, then its pre-ReLU values of y1 r2, x1 r3, y2 r4 and
// x2 r5: 9 + 25 + 49 + 81 + 121 = 285 positions x 512 B (counted in halves)
constexpr int PV_PATCH_POS = 285;
constexpr int PV_PATCH_HALVES = PV_PATCH_POS * 256;
// Of a root's maps only x0 is stored (conv0's reference of its children); y1, x1, y2 are
// relu of the pre-ReLU values and nothing reads them.  The patch slots share one pool:
// per root map slot the bytes of those three maps and of the 16 patches of 164 positions
// that the workspace held before the patches grew -- so gz_pv_tree_workspace_bytes is what
// it was, and the pool holds 11.9 patch slots per root map slot
constexpr size_t PV_PATCH_POOL_BYTES = 3 * (size_t)PV_MAP_HALVES * 2 + 16 * (size_t)164 * 512;
// tree scratch per grid entry (one per CU): PV_SCRATCH_AREAS areas of a node's D
// squares (x0 r1, y1 r2, x1 r3, y2 r4: 164 positions x 256 halves), shared by the
// workgroups of pv_dg_kernel on that entry (it static_asserts its need against it)
constexpr int PV_SCRATCH_AREAS = 12;
constexpr int PV_SCRATCH_AREA_HALVES = 164 * 256;
// per-board record of the 1x1 head convs' outputs between the tower and the FC heads
// (gz_pvnet.hip / gz_pvinc.hip -> pv_heads_kernel): hp [0, 450) channel-major, zero to
// HP_K; hv [HV_OFF, HV_OFF + 225), zero to HSTRIDE
constexpr int HP_K = 464, HV_OFF = HP_K, HV_K = 240, HSTRIDE = HV_OFF + HV_K;
// the f16x3 heads' fp16 B fragments (gz_pvnet.hip, pv_heads_pack_kernel): policy_fc
// then value_fc1, [kb][n-tile][lane][8], a hi plane then a lo plane
constexpr int HF_PKB = 15, HF_VKB = 8;  // k-blocks: policy 480 >= 450 inputs, value 256 >= 225
constexpr int HF_VAL = HF_PKB * PF_NT * 64 * 8;             // halves: value_fc1's fragments
constexpr int HF_PLANE = HF_VAL + HF_VKB * V1_NT * 64 * 8;  // halves per plane (hi, lo)
constexpr size_t HF_BYTES = 2 * (size_t)HF_PLANE * sizeof(_Float16);

// algorithmic work of one forward (neural_network.py:132-159), MACs
constexpr long long MACS = 133690114LL;

// ---------------------------------------------------------------- tree forward (host)
// The counter block of a tree forward (TreeWs::ctr, zeroed by gz_internal_tree_classify):
// list counts, then the 16-row MFMA tile-taps the incremental kernel executed, then the
// per-XCD chunk queue heads of pv_dg_kernel's two launches
enum TreeCtr {
    CTR_ROOTS_SEEN = 0,  // leaves tagged as roots (with or without a map slot)
    CTR_ROOTS = 1,       // roots with a map slot: full forward, maps stored
    CTR_CHILDREN = 2,    // root children (pv_dg_kernel)
    CTR_FULL = 3,        // every other board without a stored root or patch: full forward
    CTR_GRAND = 4,       // grandchildren (pv_dg_kernel, the overlay form)
    CTR_PATCHES = 5,     // patch slots claimed
    CTR_STATS = 6,       // gz_pv_tree_stats copies [0, CTR_STATS)
    CTR_TILES = 8,       // [2] executed tile-taps: root children, grandchildren
    CTR_DG_QUEUE = 16,   // [8] pv_dg_kernel's queue heads, the children's launch
    CTR_GRAND_QUEUE = 24,  // [8] the same of the grandchildren's launch
    CTR_COUNT = 32
};
static_assert(CTR_STATS <= CTR_TILES && CTR_TILES + 2 <= CTR_DG_QUEUE && CTR_DG_QUEUE + 8 == CTR_GRAND_QUEUE &&
                  CTR_GRAND_QUEUE + 8 == CTR_COUNT, "counter slots");

constexpr size_t al256(size_t x) { return (x + 255) & ~(size_t)255; }
constexpr int32_t patch_cap_of(int32_t root_cap) {
    return (int32_t)((size_t)(root_cap < 0 ? 0 : root_cap) * PV_PATCH_POOL_BYTES / ((size_t)PV_PATCH_HALVES * 2));
}

// The tree-forward workspace, described once: byte offsets of its regions for n leaves,
// root_cap root map slots and `grid` scratch entries (one per CU), in order; `end` is
// gz_pv_tree_workspace_bytes.  tree_carve (gz_pvnet.hip) applies them to the base pointer.
struct TreeLayout {
    size_t hbuf;      // [n][HSTRIDE] f32 head-conv records
    size_t ord, pslot, roots, full, grand, gnext, cinfo;  // [n] i32 each
    size_t children;  // [n] i32 + the per-wave counts of tree_lists_kernel [n / 64 + 1]
    size_t ctr;       // [CTR_COUNT] i32
    size_t ghead;     // [16 root_cap >= patch_cap] i32
    size_t maps;      // [root_cap][PV_MAP_HALVES] f16: x0
    size_t pres;      // [root_cap][4][PV_PRE_FLOATS] f32
    size_t patches;   // [patch_cap][PV_PATCH_POS][128] f32
    size_t scratch;   // [grid][PV_SCRATCH_AREAS][PV_SCRATCH_AREA_HALVES] f16
    size_t hf;        // HF_BYTES
    size_t end;
};
constexpr TreeLayout tree_layout(int32_t n, int32_t root_cap, int grid) {
    const size_t m = (size_t)(n < 1 ? 1 : n), rc = (size_t)(root_cap < 0 ? 0 : root_cap);
    TreeLayout l{};
    size_t p = 0;
    const auto take = [&p](size_t bytes) {
        const size_t at = p;
        p += bytes;
        return at;
    };
    l.hbuf = take(al256(m * HSTRIDE * sizeof(float)));
    for (size_t* a : {&l.ord, &l.pslot, &l.roots, &l.full, &l.grand, &l.gnext, &l.cinfo}) *a = take(al256(m * 4));
    l.children = take(al256((m + m / 64 + 1) * 4));
    l.ctr = take(al256(CTR_COUNT * sizeof(int32_t)));
    l.ghead = take(al256(16 * rc * 4));
    l.maps = take(rc * PV_MAP_HALVES * sizeof(_Float16));
    l.pres = take(rc * 4 * PV_PRE_FLOATS * sizeof(float));
    l.patches = take(rc * PV_PATCH_POOL_BYTES);
    l.scratch = take((size_t)grid * PV_SCRATCH_AREAS * PV_SCRATCH_AREA_HALVES * sizeof(_Float16));
    l.hf = take(HF_BYTES);
    l.end = p;
    return l;
}

// the carved workspace: what gz_internal_tree_classify / _children / _delta work on
struct TreeWs {
    float* hbuf;
    int32_t *ord, *pslot, *roots, *full, *grand, *gnext, *cinfo, *children, *ghead, *ctr;
    _Float16* maps;
    float* pres;        // the roots' pre-BN accumulators (pv_dg_kernel)
    float* patches;     // the parents' patches (pv_dg_kernel)
    _Float16* scratch;  // pv_dg_kernel: PV_SCRATCH_AREAS areas per grid entry
    _Float16* hf;       // the heads' fp16 fragments
    int32_t patch_cap;
};
}  // namespace gzpv
