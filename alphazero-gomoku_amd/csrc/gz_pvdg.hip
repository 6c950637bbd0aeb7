// gz_pvdg.hip -- the root children's policy-value forward as a DELTA of the root's,
// gathered (tree mode "delta"; AlphaZeroGomokuNet, neural_network.py:74-91,132-159,
// evaluated once per node the search creates, ai_agent.py:522-523).
//
// A root child is its root plus one stone at cell m.  At the input of residual layer L
// (y1, x1, y2, x2 = L 0..3) the child's activations differ from the root's only in the
// square of radius L+1 around m, so the child's pre-BN accumulator of layer L is the
// root's plus the convolution of that difference D:
//     B_child(p) = B_root(p) + sum_t W_t * D(p + t),    p within radius L+2 of m.
// The root's full forward dumps z = BN(B_root) [+ skip] per layer (gz_pvnet.hip), so
//     child(p) = relu(z(p) + s * sum_t W_t D(p + t) + D_skip(p)),
// and the next layer's D = child - relu(z).  Outputs stay within the f32 rounding of
// a full forward (tests/test_gpu_pvdelta.py: 2e-5 of the full forward, 1e-4 of the
// reference), not bitwise.
//
// Schedule (K below): two workgroups per CU, each (4 waves, one per SIMD) taking chunks
// of 6 consecutive root children (a root's children are adjacent in the list): y1 over
// the 6 nodes, x1 over 3 + 3, then per node pair y2 over the pair and x2 + the 1x1 heads
// over each node -- 12 passes per 6 nodes, each pass one stream of a layer's 576 KB of
// hi/lo weight fragments for up to 12 16-row tiles.
//
// Gather with tap skipping: a pass's output rows (every on-board position of each
// node's radius-(L+2) square) are MFMA M rows; row p needs tap t only if p + t lies in
// the D square (and on the board) -- a set TY x TX.  The rows are counting-sorted by
// that class in an order that puts each tap set next to its supersets (gz_dgclass.h),
// so a 16-row tile's tap set (the union of its rows') is small, and a tile runs only
// its taps: 95 tile-taps per node on real searches (92 for the unclipped
// ideal), against 124 for the exact recomputation of the squares -- the delta
// form's saving without pv_delta_kernel's scatter (an LDS read-add-write of the
// accumulators per tap).  Accumulators stay in registers for the whole pass; the D
// squares of the pass's nodes sit in LDS ([plane][16 cg][position][8], a node's square
// row-major, a zero slot for the taps a row does not need), read per tap at the row's
// position + the tap's offset.
//
// Between layers each node's D squares (x0 r1, y1 r2, x1 r3, y2 r4: the patch layout)
// go to the workgroup's scratch in global memory and come back by LDS-DMA for the
// passes that read them -- except where the next pass is the next layer of the same
// first nodes (y1 -> x1 of nodes 0-2, y2 -> x2 of node 2k): those squares go from the
// epilogue straight into the next pass's LDS image.  A node with grandchildren also
// writes its pre-ReLU values of the squares (and x2's, radius 5) into its patch slot in
// fp32, position-major: a lane's 8 channels are 32 contiguous bytes of a row.
//
// Grandchildren (OVERLAY instantiation, a second launch over t.grand): G = C + a stone
// at m2, C = R + a stone at m1, evaluated as a delta of the parent C exactly as above,
//     G(p) = relu(z_C(p) + s * sum_t W_t D(p + t) + D_skip(p)),   D_next = G - relu(z_C),
// where z_C is C's patch row inside C's changed square (radius L + 2 around m1) and the
// root's z elsewhere (fp32: a channel the ReLU clipped in C can be lifted by G's delta);
// conv0's reference x0 is C's within radius 1 of m1; the record's base is C's record.
// Everything else -- rows, classes, k-loop, fills, scratch, queue -- is the children's code.
// A lane owns the 8 channels of one 16-byte slot of those layouts (dg_ch0 below), so
// per row and plane each of these is ONE 16-byte access: the D store, the patch store,
// the LDS hand-off write, the skip load and conv0's root-x0 load.
#include <hip/hip_runtime.h>

#include <cstdlib>
#include <type_traits>

#include "gz_dgclass.h"
#include "gz_internal.h"
#include "gz_pvtree.h"

using namespace gzpv;

namespace {

using namespace gzc;

constexpr int NTD = 256;  // 4 waves
#ifndef GZ_DG_NTE
#define GZ_DG_NTE 1
#endif
__host__ __device__ constexpr int dg_s(int L) { return 2 * L + 3; }  // D-square width (radius L+1)
__host__ __device__ constexpr int dg_ss(int L) { return dg_s(L) * dg_s(L); }
__host__ __device__ constexpr int dg_so(int L) { return 2 * L + 5; }  // output-square width (radius L+2)

// Schedule: two workgroups per CU (<= 80 KB of LDS and <= 256 registers each), so that
// one workgroup's epilogue, fills and barriers run beside the other's MFMAs.  A
// workgroup takes chunks of 6 consecutive nodes; passes of 6 / 3 / 2 / 1 nodes (y1 / x1 /
// y2 / x2), up to 12 output tiles each.  (One workgroup per CU with chunks of 12 and
// passes of 12 / 6 / 4 / 3 -- 87.5 instead of 102 tile-taps per node, but the serial
// phases exposed -- measured 146 against 126 ms per tree forward.)
__host__ __device__ constexpr int dgk_g(int L) { return L == 0 ? 6 : (L == 1 ? 3 : (L == 2 ? 2 : 1)); }
__host__ __device__ constexpr int dgk_npos(int L) { return (dgk_g(L) * dg_ss(L) + 1 + 15) & ~15; }
struct K {
    static constexpr int C = 6;  // nodes per chunk
    __host__ __device__ static constexpr int g(int L) { return dgk_g(L); }
    static constexpr int NPASS = 1 + C / 3 + C / 2 + C;
    // the pass of layer L that takes node gi: y1, x1 x 2, then per node pair k: y2(2k, 2k+1),
    // x2(2k), x2(2k+1) -- so that node 2k's D(y2) goes from the y2 epilogue straight into
    // the x2 pass's LDS image (layer-major y2 x 3, x2 x 6: 1.8 % slower, profiles/r06/ab.md)
    __host__ __device__ static constexpr int pass_of(int L, int gi) {
        return L == 0 ? 0 : (L == 1 ? 1 + gi / 3 : (L == 2 ? 3 + 3 * (gi / 2) : 4 + 3 * (gi / 2) + (gi & 1)));
    }
    // positions of a pass's LDS image: the nodes' squares back to back, then at least one
    // zero slot (the last), rounded to 16 so that a channel group's plane starts at bank 0
    __host__ __device__ static constexpr int npos(int L) { return dgk_npos(L); }
    static constexpr int MAXNPOS = 112;            // npos(2) = max over the layers (static_assert below)
    static constexpr int NMAX = 12;                // output tiles of a pass at most (y2: 2 x 81 rows in 11)
    static constexpr int ROWS = NMAX * 16;         // row-table entries per pass
    static constexpr int GB = 2;                   // epilogue: tiles per load group
    static constexpr int WPS = 2;                  // workgroups per CU
    static constexpr int NKEY = 36;                // row classes (6 x 6 tap sets)
    // LDS
    static constexpr int IN = 0;                   // D squares [2 planes][16 cg][NPOS][8] halves
    static constexpr int IN_BYTES = 32 * MAXNPOS * 16;
    static constexpr int COL = 32 * dgk_npos(0) * 16;  // conv0's im2col (chunk start), behind the y1 image
    static constexpr int HP = IN + IN_BYTES;       // x2: head partials [g(3) nodes][4 waves][3][121] f32
    static constexpr int HP_BYTES = dgk_g(3) * 4 * 3 * 121 * 4;
    static constexpr int ROWT = HP + HP_BYTES;     // row tables [NPASS][ROWS] u32
    static constexpr int MASK = ROWT + NPASS * ROWS * 4;  // [NPASS][16] u32: tap masks [0, 9), rows [9], tile-taps [10]
    static constexpr int HIST = MASK + NPASS * 16 * 4;    // class counters [NPASS][36] (zero between uses), then starts
    static constexpr int U = HIST + 2 * NPASS * NKEY * 4;  // units
    static constexpr int CST = U + C * 128;        // BN scales of the 4 residual layers [4][128], the 1x1 head
    static constexpr int CST_FLOATS = 4 * 128 + 3 * 128 + 4;  // weights [3][128], the 3 head biases
    static constexpr int POS = CST + CST_FLOATS * 4;  // the chunk's first list entry and its queue's end (int)
    static constexpr int LDS = POS + 16;
};
static_assert(dgk_npos(0) <= K::MAXNPOS && dgk_npos(1) <= K::MAXNPOS && dgk_npos(2) == K::MAXNPOS &&
                  dgk_npos(3) <= K::MAXNPOS, "image");
static_assert(K::LDS * K::WPS <= 160 * 1024, "LDS budget");
static_assert(K::COL + K::C * 1024 <= K::IN_BYTES, "im2col behind the y1 image");
static_assert(dgk_g(0) * dg_so(0) * dg_so(0) <= K::ROWS && dgk_g(1) * dg_so(1) * dg_so(1) <= K::ROWS &&
                  dgk_g(2) * dg_so(2) * dg_so(2) <= K::ROWS && dgk_g(3) * dg_so(3) * dg_so(3) <= K::ROWS, "rows");
static_assert(K::C % 6 == 0 && dgk_g(3) == 1, "passes; one x2 node per pass (the record prefetch)");
static_assert(K::C == 6 && dgk_g(1) == 3 && dgk_g(2) == 2, "pass order (K::pass_of, dg_pass_of): 2 x1 triples, 3 y2 pairs");

// The workgroup's scratch: the D squares that cross passes, each map's squares in a
// region of their own ([2 planes][16 cg][square][8] halves per node), sized by what is
// live at once in the pass order -- x0 r1 of the 6 nodes (to the x1 passes' skip), x1 r3
// of the 6 (to the y2 passes and the x2 skip), and one region shared by y1 r2 of nodes
// 3..5 (the first x1 pass takes nodes 0..2's from LDS; dead after the second x1 pass) and
// y2 r4 of node 2k + 1 (node 2k's goes through LDS; dead after x2(2k + 1), before the next
// pair's y2 writes).  429 positions x 512 B = 215 KiB per workgroup instead of 6 patch
// layouts (504 KiB): less to evict from L2 per chunk.
__host__ __device__ constexpr int scr_sq(int map, int node) {
    return (map == 0 ? 9 * node : (map == 2 ? 54 + 49 * node : (map == 1 ? 348 + (node >= 3 ? 25 * (node - 3) : 0) : 348))) * 256;
}
constexpr int SCR_HALVES = (348 + 81) * 256;
static_assert(348 + 3 * 25 <= 348 + 81 && 54 + 49 * 6 == 348, "scratch regions");

struct DgUnit {
    const _Float16* gm;  // the root's x0 map (hi / lo)
    const float* pre;    // the root's pre-ReLU values of y1, x1, y2, x2
    _Float16* own;       // the workgroup's scratch: this node's D square of map k at own + sq[k]
    float* patch;        // a child's own patch slot (or nullptr); a grandchild's PARENT's patch
    int leaf, base, cell, pcell;  // node, record base (root / parent), stone; grandchild: the parent's stone
    int sq[4];           // halves offsets of its D squares x0 r1, y1 r2, x1 r3, y2 r4 (scr_sq)
    uint32_t board[16];  // the node's bit-plane board (conv0's input)
};
static_assert(sizeof(DgUnit) == 128, "unit size");

struct DgArgs {
    const int32_t* cinfo;  // per leaf: (root map slot << 8) | stone cell (tree_lists_kernel)
    const float* W;
    const uint32_t* boards;
    const int32_t* meta;
    const int32_t* pslot;
    const _Float16* maps;
    const float* pres;
    float* patches;
    float* hbuf;
    int32_t* tiles;  // += executed tile-taps (one 16-row tile x one tap x 128 x 128)
    int32_t* queue;  // [8] per-XCD chunk heads, zero at the launch
};

// Phase stamps (-DGZ_PVDG_STAMPS builds, tools/pvinc_bench.py).  Phases: 0 chunk start (units, conv0, rows of y1), 1 rows of the next pass, 2..5 the
// k-loops of y1 / x1 / y2 / x2, 6 the barrier after a k-loop, 7..10 the epilogues,
// 11 store drain + barrier, 12 records, 13 fill + barrier
#ifdef GZ_PVDG_STAMPS
__device__ unsigned long long gz_pvdg_stamps[16];
__device__ unsigned long long gz_pvdg_stamps_n[1];
using DgStamp = PhaseStamp<gz_pvdg_stamps>;
#else
using DgStamp = PhaseStamp<nullptr>;
#endif

// global-memory accesses through the unit table's pointers as global (not flat)
// instructions: flat ones count against lgkmcnt too and would hold the LDS waits
#define GZ_GLB __attribute__((address_space(1)))
#ifdef GZ_DG_CHK
// debug builds (tools only): every global access of the kernel checked against the tree
// workspace's bounds; an access outside is counted and redirected to the workspace start
__device__ unsigned long long gz_dg_chk[16];
__device__ const char* gz_dg_lo;
__device__ const char* gz_dg_hi;
__device__ __forceinline__ const void* dg_chk(const void* p, int code) {
    if ((const char*)p < gz_dg_lo || (const char*)p >= gz_dg_hi) {
        atomicAdd(&gz_dg_chk[code], 1ull);
        return gz_dg_lo;
    }
    return p;
}
#define DG_CHK(p, code) dg_chk((p), (code))
#else
#define DG_CHK(p, code) (p)
#endif
template <class T>
__device__ __forceinline__ T gld(const void* p) {
    return *(const GZ_GLB T*)DG_CHK(p, 0);
}
template <class T>
__device__ __forceinline__ void gst(void* p, const T& v) {
    *(GZ_GLB T*)DG_CHK(p, 1) = v;
}

// ------------------------------------------------------------------ lanes and channels
// Wave np's two n-tiles cover channels [32 np, 32 np + 32).  Of n-tile n, lane (q = lane
// >> 4) holds the accumulators of channels 32 np + 8 q + 4 n + r, r = 0..3: with both
// n-tiles the 8 channels of ONE 16-byte slot of the [plane][16 cg][position][8] layouts
// (channel group 4 np + q), so every D / patch / image store and every skip / x0 load of a
// row is one 16-byte access per plane.  (In channel order, (2 np + n) * 16 + 4 q + r, a
// lane held half of two slots: twice the instructions, 8 bytes each.)
// MFMA output row i = 4 q + r of n-tile n is then channel 32 np + 8 (i >> 2) + 4 n + (i & 3),
// so A-operand lane l (i = l & 15) holds that channel's weights -- in the fragment arrays
// (F16_RES0, F16_C0: [k-step][n-tile][lane][8] halves, channel order) n-tile 2 np + (i >> 3),
// lane (l & 48) | (8 ((i >> 2) & 1) + 4 n + (i & 3)): a wave still reads its 2 KB per k-step.
__device__ __forceinline__ int dg_ch0(int np, int q, int n) { return 32 * np + 8 * q + 4 * n; }
// the lane's fragment ([n-tile][lane] index) of n-tile 0; n-tile 1's is DG_WFRAG_N further
__device__ __forceinline__ int dg_wfrag(int np, int lane) {
    const int i = lane & 15;
    return (2 * np + (i >> 3)) * 64 + ((lane & 48) | (8 * ((i >> 2) & 1) + (i & 3)));
}
constexpr int DG_WFRAG_N = 4;

// ------------------------------------------------------------------ rows of a pass
// row entry: node (4 bits) | dy + RO (4) << 4 | dx + RO (4) << 8 | tap mask (9) << 12 |
// valid << 21; tap bit (ty + 1) * 3 + (tx + 1)
// class rank of the row's tap sets: dg_class_rank (gz_dgclass.h)

// The row tables of every pass of the chunk (nodes U[0, ng)), counting-sorted by class,
// then per pass and tap the tiles that need it.  Ends with the tables written but NOT
// published (the caller's next barrier does).
__device__ __forceinline__ void dg_rows_all(char* lds, const DgUnit* U, int ng, int tid) {
    uint32_t* hist = (uint32_t*)(lds + K::HIST);  // [NPASS][36] counters, then [NPASS][36] starts
    uint32_t* starts = hist + K::NPASS * K::NKEY;
    uint32_t* rt0 = (uint32_t*)(lds + K::ROWT);
    uint32_t* mk0 = (uint32_t*)(lds + K::MASK);
    // candidates: layer-major, then node, then position of the node's output square
    constexpr int N0 = 25, N1 = 49, N2 = 81, N3 = 121;
    const int o1 = ng * N0, o2 = o1 + ng * N1, o3 = o2 + ng * N2, tot = o3 + ng * N3;
    constexpr int PER = (K::C * (N0 + N1 + N2 + N3) + NTD - 1) / NTD;
    int kk[PER], rank[PER];
    uint32_t ent[PER];
#pragma unroll
    for (int i = 0; i < PER; i++) {
        const int c = tid + i * NTD;
        kk[i] = -1;
        rank[i] = 0;
        ent[i] = 0;
        if (c >= tot) continue;
        const int L = c < o1 ? 0 : (c < o2 ? 1 : (c < o3 ? 2 : 3));
        const int SO = 2 * L + 5, RO = L + 2, RIN = L + 1;
        const int cl = c - (L == 0 ? 0 : (L == 1 ? o1 : (L == 2 ? o2 : o3)));
        const int gi = cl / (SO * SO), j = cl - gi * (SO * SO), dy = j / SO - RO, dx = j - (j / SO) * SO - RO;
        const int cell = U[gi].cell, cr = cell / BN, cc = cell - (cell / BN) * BN;
        const int pr = cr + dy, pc = cc + dx;
        if (pr < 0 || pr >= BN || pc < 0 || pc >= BN) continue;
        int ty = 0, tx = 0;
#pragma unroll
        for (int d = -1; d <= 1; d++) {
            const int qy = dy + d, qx = dx + d;
            if (qy >= -RIN && qy <= RIN && cr + qy >= 0 && cr + qy < BN) ty |= 1 << (d + 1);
            if (qx >= -RIN && qx <= RIN && cc + qx >= 0 && cc + qx < BN) tx |= 1 << (d + 1);
        }
        if (!ty || !tx) continue;
        uint32_t m = 0;
#pragma unroll
        for (int a = 0; a < 3; a++)
            if ((ty >> a) & 1) m |= (uint32_t)tx << (3 * a);
        const int gl = L == 0 ? 0 : (L == 1 ? 3 : (L == 2 ? 2 : 1));  // nodes per pass of layer L (g(L))
        const int p = K::pass_of(L, gi), u0 = L == 0 ? 0 : (gi / gl) * gl;
        kk[i] = p * K::NKEY + dg_class_rank(ty, tx);
        ent[i] = (uint32_t)(gi - u0) | ((uint32_t)(dy + RO) << 4) | ((uint32_t)(dx + RO) << 8) | (m << 12) | (1u << 21);
        rank[i] = (int)atomicAdd(&hist[kk[i]], 1u);
    }
    __syncthreads();
    {  // wave w: the bucket starts of passes w, w + 4, ... (exclusive scans of 36 counters), counters back to 0
        const int w = tid >> 6, ln = tid & 63;
        for (int p = w; p < K::NPASS; p += NTD / 64) {
            const uint32_t v = ln < K::NKEY ? hist[p * K::NKEY + ln] : 0u;
            uint32_t x = v;
#pragma unroll
            for (int d = 1; d < 64; d <<= 1) {
                const uint32_t y = __shfl_up(x, d);
                if (ln >= d) x += y;
            }
            if (ln < K::NKEY) {
                starts[p * K::NKEY + ln] = x - v;
                hist[p * K::NKEY + ln] = 0u;
            }
            if (ln == 63) mk0[p * 16 + 9] = x;
        }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < PER; i++)
        if (kk[i] >= 0) rt0[(kk[i] / K::NKEY) * K::ROWS + starts[kk[i]] + rank[i]] = ent[i];
    for (int e = tid; e < K::NPASS * K::ROWS; e += NTD)
        if ((uint32_t)(e % K::ROWS) >= mk0[(e / K::ROWS) * 16 + 9]) rt0[e] = 0u;
    __syncthreads();
    {  // wave w, passes w, w + 4, ...: tile tap sets (union of the tile's rows), then per tap the tiles
        const int w = tid >> 6, ln = tid & 63;
        for (int p = w; p < K::NPASS; p += NTD / 64) {
            const uint32_t* rt = rt0 + p * K::ROWS;
            uint32_t tm = 0;
            if (ln < K::NMAX)
#pragma unroll
                for (int k = 0; k < 16; k++) tm |= (rt[ln * 16 + k] >> 12) & 0x1ffu;
            int exec = 0;
#pragma unroll
            for (int t = 0; t < 9; t++) {
                const uint64_t b = __ballot((tm >> t) & 1u);
                if (ln == 0) mk0[p * 16 + t] = (uint32_t)b;
                exec += __popcll(b);
            }
            if (ln == 0) mk0[p * 16 + 10] = (uint32_t)exec;
        }
    }
}

// ------------------------------------------------------------------ the k-loop
// The pass's residual conv for the wave's two n-tiles (wave nt0 / 2's 32 channels in the
// lane order of dg_ch0, the weight fragments picked by dg_wfrag) over NT output tiles:
// per tap, per 32-channel k-step (the full kernel's k order and its 3 products:
// w_hi a_hi, w_lo a_hi, w_hi a_lo), the tiles that need the tap.  ri[m]: the lane's row
// of tile m: (D-square index of its position + 32) | tap mask << 16.  Activation
// fragments are read one tile ahead unconditionally (deterministic LDS counters: the
// MFMAs of tile m wait only for its own reads), MFMAs only where the tile needs the tap;
// weight fragments through a 4-deep ring refilled 3 k-steps ahead.
template <int NT, int L>
__device__ __forceinline__ void dg_kloop(const char* lds, const uint32_t (&ri)[K::NMAX], const uint32_t* mk,
                                         const _Float16* __restrict__ Wf, int nt0, int lane,
                                         f32x4 (&acc)[2][K::NMAX]) {
    constexpr int S = dg_s(L), NPOS = K::npos(L), CQ = 4, KS = 9 * CQ;
    constexpr int CQB = 4 * NPOS * 16, PLB = 16 * NPOS * 16, ZIDX = NPOS - 1;
    constexpr int KS_BYTES = 8 * 64 * 8 * 2, LO_BYTES = KS * KS_BYTES, RING = 4;
    const int lb = K::IN + (lane >> 4) * NPOS * 16;
    const __amdgpu_buffer_rsrc_t wr = __builtin_amdgcn_make_buffer_rsrc((void*)Wf, 0, 0x7fffffff, 0x00020000);
    const int wo = dg_wfrag(nt0 >> 1, lane) * 16;
    auto wload = [&](int ks, int n, int lo) -> h8 {
        return __builtin_bit_cast(h8, __builtin_amdgcn_raw_buffer_load_b128(wr, wo, ks * KS_BYTES + n * DG_WFRAG_N * 16 + lo * LO_BYTES, 0));
    };
    auto addr = [&](int tap, uint32_t r) -> int {
        const int toff = (tap / 3 - 1) * S + (tap - (tap / 3) * 3 - 1);
        const bool v = (r >> (16 + tap)) & 1u;
        return lb + (v ? (int)(r & 0xffffu) - 32 + toff : ZIDX) * 16;
    };
    // Units of two k-steps (a tap's channels 0-63 or 64-127): per tile 12 MFMAs behind one
    // test of the tile's tap mask (with one k-step per unit the per-tile reads, the test
    // and the waits took a third of the loop).  Weights: a ring of 4 k-steps = 2 units,
    // the next unit's pair loaded at the start of a unit into the pair the previous unit
    // released.  Fragments one tile ahead, read unconditionally (the LDS counter is then
    // the same on every path: a tile's MFMAs wait only for its own reads).
    h8 b[RING][2][2];
#pragma unroll
    for (int c = 0; c < 2; c++)
#pragma unroll
        for (int n = 0; n < 2; n++) {
            b[c][n][0] = wload(c, n, 0);
            b[c][n][1] = wload(c, n, 1);
        }
    f32x4 c[2][NT];
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
        for (int m = 0; m < NT; m++) c[n][m] = acc[n][m];
    int ad[NT];
#pragma unroll
    for (int m = 0; m < NT; m++) ad[m] = addr(0, ri[m]);
    h8 fh[2][2], fl[2][2];  // [fragment parity][k-step of the pair]
#pragma unroll
    for (int k2 = 0; k2 < 2; k2++) {
        fh[0][k2] = *(const h8*)(lds + ad[0] + k2 * CQB);
        fl[0][k2] = *(const h8*)(lds + ad[0] + k2 * CQB + PLB);
    }
#pragma unroll 1
    for (int tap = 0; tap < 9; tap++) {
        const uint32_t tm = (uint32_t)__builtin_amdgcn_readfirstlane((int)mk[tap]);
#pragma unroll
        for (int h = 0; h < 2; h++) {
            {  // the next unit's k-steps into the pair the previous unit released (past the end: unused)
                const int ksr = tap * CQ + 2 * h + 2;
                const int kn = ksr < KS ? ksr : ksr - KS;
#pragma unroll
                for (int k2 = 0; k2 < 2; k2++)
#pragma unroll
                    for (int n = 0; n < 2; n++) {
                        b[(2 * h + 2 + k2) & 3][n][0] = wload(kn + k2, n, 0);
                        b[(2 * h + 2 + k2) & 3][n][1] = wload(kn + k2, n, 1);
                    }
            }
#pragma unroll
            for (int m = 0; m < NT; m++) {
                // (NT is even: a unit reads an even number of fragment pairs, so tile m's
                // parity is m & 1 on every tap)
                const int pm = m & 1, pn = (m + 1) & 1;
                // the next tile's pair: tile m + 1, else tile 0 of the next unit (the second
                // half of this tap, or the next tap's first, whose address ad[0] holds)
                int na;
                if (m + 1 < NT) na = ad[m + 1] + 2 * h * CQB;
                else na = h == 0 ? ad[0] + 2 * CQB : ad[0];
#pragma unroll
                for (int k2 = 0; k2 < 2; k2++) {
                    fh[pn][k2] = *(const h8*)(lds + na + k2 * CQB);
                    fl[pn][k2] = *(const h8*)(lds + na + k2 * CQB + PLB);
                }
                if (h == 1) ad[m] = addr(tap + 1, ri[m]);  // tile m is read for this tap: the next tap's address
                if ((tm >> m) & 1u) {
#pragma unroll
                    for (int k2 = 0; k2 < 2; k2++) {
                        const int sl = 2 * h + k2;
                        const h8 ah = fh[pm][k2], al = fl[pm][k2];
#pragma unroll
                        for (int n = 0; n < 2; n++) c[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b[sl][n][0], ah, c[n][m], 0, 0, 0);
#pragma unroll
                        for (int n = 0; n < 2; n++) c[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b[sl][n][1], ah, c[n][m], 0, 0, 0);
#pragma unroll
                        for (int n = 0; n < 2; n++) c[n][m] = __builtin_amdgcn_mfma_f32_16x16x32_f16(b[sl][n][0], al, c[n][m], 0, 0, 0);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
        for (int m = 0; m < NT; m++) acc[n][m] = c[n][m];
}

// ------------------------------------------------------------------ epilogue
// a 16-byte slot (the lane's 8 channels: n-tile 0's four, then n-tile 1's), hi and lo planes
struct H8x2 {
    h8 h, l;
};
__device__ __forceinline__ float h2f(const H8x2& x, int r) { return (float)x.h[r] + (float)x.l[r]; }
// the lane's values of both n-tiles split into hi / lo halves
__device__ __forceinline__ H8x2 split_hl(const f32x4 (&v)[2]) {
    H8x2 o;
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
        for (int r = 0; r < 4; r++) {
            const _Float16 h = (_Float16)v[n][r];
            o.h[4 * n + r] = h;
            o.l[4 * n + r] = (_Float16)(v[n][r] - (float)h);
        }
    return o;
}
// a slot at p (global memory), its lo plane at p + plane_halves
__device__ __forceinline__ void put_hl(_Float16* p, int plane_halves, const H8x2& x) {
    gst<h8>(p, x.h);
    gst<h8>(p + plane_halves, x.l);
}
// the lane's 8 channels in fp32 at p (a patch row: 32 contiguous bytes)
__device__ __forceinline__ void put_f8(float* p, const f32x4 (&v)[2]) {
    gst<f32x4>(p, v[0]);
    gst<f32x4>(p + 4, v[1]);
}
// the same into LDS
__device__ __forceinline__ void put_hl_lds(_Float16* p, int plane_halves, const H8x2& x) {
    *(h8*)p = x.h;
    *(h8*)(p + plane_halves) = x.l;
}

// The epilogue of a pass (layer L, nodes U[0, g), row table rt): per row,
//   child = relu(z + s * acc + D_skip),  root = relu(z),  D = child - root
// into the node's D square of map L + 1 (its patch: the pre-ReLU value); x2 reduces the
// child values into the 1x1 heads' partial sums (hpart, per wave) instead.  Rows in
// groups of GB tiles, loads ST - 1 groups ahead.
// OVERLAY (a grandchild, the delta of its parent): z is the parent's -- its patch row
// inside its changed square (radius L + 2 around its stone), the root's elsewhere --
// and nothing is written to a patch.
template <int L, bool OVERLAY>
__device__ __forceinline__ void dg_epilogue(char* lds, const DgUnit* U, const uint32_t* rt, int np, int lane,
                                            const f32x4 (&acc)[2][K::NMAX], int nt, int ldsg) {
    constexpr int RO = L + 2, SO = dg_so(L), SSO = SO * SO;
    constexpr bool SKIP = L == 1 || L == 3;
    constexpr int RS = L == 1 ? 1 : 3, SK = 2 * RS + 1, SSK = SK * SK;
    constexpr int GB = K::GB, NGRP = (K::NMAX + GB - 1) / GB, ST = 2;
    float* hpart = (float*)(lds + K::HP);
    const int q = lane >> 4, li = lane & 15, cg = 4 * np + q;  // cg: the lane's channel group (dg_ch0 >> 3)
    const float* cst = (const float*)(lds + K::CST);  // staged at kernel start
    f32x4 es[2], e0[2], e1[2], ev[2];
#pragma unroll
    for (int n = 0; n < 2; n++) {
        const int ch0 = dg_ch0(np, q, n);
        es[n] = *(const f32x4*)(cst + L * 128 + ch0);
        if (L == 3) {
            e0[n] = *(const f32x4*)(cst + 512 + ch0);
            e1[n] = *(const f32x4*)(cst + 640 + ch0);
            ev[n] = *(const f32x4*)(cst + 768 + ch0);
        }
    }
    f32x4 z[ST][GB][2];
    H8x2 dk[ST][GB];
    uint32_t ent[ST][GB];
    auto loads = [&](int grp, int st) {
#pragma unroll
        for (int j = 0; j < GB; j++) {
            const int m = grp * GB + j;
            if (m >= K::NMAX) break;  // (an odd NMAX: the last group's second tile)
            const uint32_t e = rt[m * 16 + li];
            ent[st][j] = e;
            const int gi = e & 15, dy = (int)((e >> 4) & 15) - RO, dx = (int)((e >> 8) & 15) - RO;
            const DgUnit& u = U[gi];
            const int cell = u.cell, cr = cell / BN, cc = cell - (cell / BN) * BN;
            const bool v = (e >> 21) & 1u;
            const int pos = v ? (cr + dy) * BN + (cc + dx) : 0;
            const bool near = SKIP && v && iabs(dy) <= RS && iabs(dx) <= RS;
            const int sidx = near ? (dy + RS) * SK + (dx + RS) : 0;
            const float* zp = u.pre + L * PV_PRE_FLOATS + pos * CH;
            if (OVERLAY) {
                const int pcell = u.pcell, r1 = pcell / BN, c1 = pcell - (pcell / BN) * BN;
                const int oy = cr + dy - r1, ox = cc + dx - c1;
                if (v && iabs(oy) <= RO && iabs(ox) <= RO)
                    zp = u.patch + (PATCH_POS[L + 1] + (oy + RO) * SO + (ox + RO)) * CH;
            }
#pragma unroll
            for (int n = 0; n < 2; n++) z[st][j][n] = gld<f32x4>(zp + dg_ch0(np, q, n));
            if (SKIP) {
                const _Float16* p = u.own + u.sq[L - 1] + (cg * SSK + sidx) * 8;
                dk[st][j] = H8x2{gld<h8>(p), gld<h8>(p + 16 * SSK * 8)};
            }
        }
    };
#pragma unroll
    for (int grp = 0; grp < ST - 1; grp++)
        if (grp * GB < nt) loads(grp, grp);
#pragma unroll
    for (int grp = 0; grp < NGRP; grp++) {
        if (grp * GB >= nt) break;
        const int st = grp % ST;
        if ((grp + ST - 1) * GB < nt) loads(grp + ST - 1, (grp + ST - 1) % ST);
#pragma unroll
        for (int j = 0; j < GB; j++) {
            const int m = grp * GB + j;
            if (m >= K::NMAX) break;
            const uint32_t e = ent[st][j];
            const bool v = (e >> 21) & 1u;
            const int gi = e & 15, dy = (int)((e >> 4) & 15) - RO, dx = (int)((e >> 8) & 15) - RO;
            const bool near = SKIP && iabs(dy) <= RS && iabs(dx) <= RS;
            const int oidx = (dy + RO) * SO + (dx + RO);
            float s0 = 0.f, s1 = 0.f, sv = 0.f;
            f32x4 y[2], d[2];
#pragma unroll
            for (int n = 0; n < 2; n++) {
#pragma unroll
                for (int r = 0; r < 4; r++) {
                    const float zr = z[st][j][n][r];
                    float tc = __builtin_fmaf(acc[n][m][r], es[n][r], zr);
                    if (SKIP) tc += near ? h2f(dk[st][j], 4 * n + r) : 0.f;
                    if (!OVERLAY) y[n][r] = tc;  // (the patch: pre-ReLU)
                    tc = tc > 0.f ? tc : 0.f;
                    if (L == 3) {
                        s0 = __builtin_fmaf(e0[n][r], tc, s0);
                        s1 = __builtin_fmaf(e1[n][r], tc, s1);
                        sv = __builtin_fmaf(ev[n][r], tc, sv);
                    } else {
                        d[n][r] = tc - (zr > 0.f ? zr : 0.f);
                    }
                }
            }
            if (L < 3 && v) {  // the lane's slot (channel group cg) of the row's position
                const DgUnit& u = U[gi];
                const H8x2 dd = split_hl(d);
                if (gi < ldsg) {  // the next pass's image (dg_fill<L + 1>'s layout)
                    constexpr int NPN = K::npos(L + 1 < 4 ? L + 1 : 3), SSN = SSO;
                    put_hl_lds((_Float16*)(lds + K::IN) + (cg * NPN + gi * SSN + oidx) * 8, 16 * NPN * 8, dd);
                } else {
                    put_hl(u.own + u.sq[L + 1] + (cg * SSO + oidx) * 8, 16 * SSO * 8, dd);
                }
                if (!OVERLAY && u.patch) put_f8(u.patch + (PATCH_POS[L + 1] + oidx) * CH + 8 * cg, y);
            }
            if (!OVERLAY && L == 3 && v) {  // a parent's x2 square (one node per x2 pass)
                float* const pp = U[0].patch;
                if (pp) put_f8(pp + (PATCH_POS[4] + oidx) * CH + 8 * cg, y);
            }
            if (L == 3) {
                s0 += __shfl_xor(s0, 16);
                s1 += __shfl_xor(s1, 16);
                sv += __shfl_xor(sv, 16);
                s0 += __shfl_xor(s0, 32);
                s1 += __shfl_xor(s1, 32);
                sv += __shfl_xor(sv, 32);
                if (lane < 16 && v) {
                    float* h = hpart + ((gi * 4 + np) * 3) * 121 + oidx;
                    h[0] = s0;
                    h[121] = s1;
                    h[242] = sv;
                }
            }
        }
    }
}

// a node's head-conv record: the radius-5 square from the partials (bias + the 4
// waves' sums), everything else the root's record (rec: this thread's entries of the
// root's record, dg_record_load)
constexpr int REC_K = (HSTRIDE + NTD - 1) / NTD;
__device__ __forceinline__ void dg_record_load(const DgUnit& u, const float* __restrict__ hbuf, float (&rec)[REC_K],
                                               int tid) {
    const float* src = (const float*)DG_CHK(hbuf + (size_t)u.base * HSTRIDE, 3);
#pragma unroll
    for (int k = 0; k < REC_K; k++) {
        const int j = tid + k * NTD;
        rec[k] = j < HSTRIDE ? src[j] : 0.f;
    }
}
__device__ __forceinline__ void dg_record(const DgUnit& u, int g, const float* bias, float* __restrict__ hbuf,
                                          const float* hpart, const float (&rec)[REC_K], int tid) {
    const int cr = u.cell / BN, cc = u.cell - (u.cell / BN) * BN;
    float* h = (float*)DG_CHK(hbuf + (size_t)u.leaf * HSTRIDE, 4);
#pragma unroll
    for (int k = 0; k < REC_K; k++) {
        const int j = tid + k * NTD;
        if (j >= HSTRIDE) break;
        float v = rec[k];
        int pos = -1, which = 0;
        if (j < POS) {
            pos = j;
        } else if (j < 2 * POS) {
            pos = j - POS;
            which = 1;
        } else if (j >= HV_OFF && j < HV_OFF + POS) {
            pos = j - HV_OFF;
            which = 2;
        }
        if (pos >= 0) {
            const int dy = pos / BN - cr, dx = pos % BN - cc;
            if (iabs(dy) <= 5 && iabs(dx) <= 5) {
                const int idx = (dy + 5) * 11 + (dx + 5);
                float a = bias[which];
#pragma unroll
                for (int w = 0; w < 4; w++) a += hpart[((g * 4 + w) * 3 + which) * 121 + idx];
                v = a;
            }
        }
        h[j] = v;
    }
}

// ------------------------------------------------------------------ fills and conv0
// the D squares of map L (L >= 1) of nodes U[0, g) into the pass's LDS image by LDS-DMA:
// a lane works out its position's source (a node's square, or zero past them) once per
// 64-position block, then wave w moves channel-group planes [8w, 8w + 8) of it -- the
// planes land at wave-contiguous LDS addresses
template <int L>
__device__ __forceinline__ void dg_fill(char* lds, const DgUnit* U, int g, int tid) {
    constexpr int SS = dg_ss(L), NPOS = K::npos(L), NB = (NPOS + 63) / 64;
    const int lane = tid & 63, wave = tid >> 6;
#pragma unroll
    for (int blk = 0; blk < NB; blk++) {
        const int idx = blk * 64 + lane;
        const _Float16* src = (const _Float16*)gz_tree_zero16;
        int stride = 0;
        if (idx < g * SS) {
            const int gi = idx / SS, j = idx - gi * SS;
            src = U[gi].own + U[gi].sq[L] + j * 8;
            stride = SS * 8;
        }
        char* dst = lds + K::IN + blk * 64 * 16;
        if (idx < NPOS) {
#pragma unroll
            for (int k = 0; k < 8; k++) {
                const int pc = wave * 8 + k;
                // (the zero source is a device global, not part of the workspace the check knows)
                const _Float16* sp = src + pc * stride;
                __builtin_amdgcn_global_load_lds((glb_void_t*)(stride ? DG_CHK(sp, 2) : sp), (lds_void_t*)(dst + pc * NPOS * 16),
                                                 16, 0, 0);
            }
        }
    }
}

// conv0's im2col for every node of the chunk (16 rows x 32 k each: the <= 9 positions
// of the radius-1 square, clipped, row-major; k = tap * 3 + cin)
__device__ __forceinline__ void dg_col(_Float16* col, const DgUnit* U, int ng, int tid) {
    for (int e = tid; e < ng * 512; e += NTD) {
        const int g = e >> 9, row = (e >> 5) & 15, k = e & 31;
        const DgUnit& u = U[g];
        const int cr = u.cell / BN, cc = u.cell - (u.cell / BN) * BN;
        const int r0 = cr > 0 ? cr - 1 : 0, r1 = cr < BN - 1 ? cr + 1 : BN - 1;
        const int c0 = cc > 0 ? cc - 1 : 0, c1 = cc < BN - 1 ? cc + 1 : BN - 1, wr = c1 - c0 + 1;
        _Float16 v = (_Float16)0.f;
        if (row < (r1 - r0 + 1) * wr && k < 27) {
            const int pr = r0 + row / wr, pc = c0 + row % wr;
            const int tap = k / 3, cin = k % 3;
            const int rr = pr + tap / 3 - 1, c2 = pc + tap % 3 - 1;
            if (rr >= 0 && rr < BN && c2 >= 0 && c2 < BN) {
                const int bit = rr * 16 + c2;
                const uint32_t bl = (u.board[bit >> 5] >> (bit & 31)) & 1u, wh = (u.board[8 + (bit >> 5)] >> (bit & 31)) & 1u;
                v = (_Float16)(float)(cin == 0 ? bl : (cin == 1 ? wh : 1u - (bl | wh)));
            }
        }
        col[e] = v;
    }
}

// conv0 + BN + ReLU at the <= 9 positions around each node's stone, D(x0) = child -
// root into the y1 pass's LDS image and the node's x0 square (its patch: the child value).
// OVERLAY: the reference x0 is the parent's -- its patch within radius 1 of its stone
template <bool OVERLAY>
__device__ __forceinline__ void dg_conv0(char* lds, const _Float16* col, const DgUnit* U, int ng,
                                         const float* __restrict__ W, int np, int lane) {
    constexpr int NPOS = K::npos(0);
    const int li = lane & 15, q = lane >> 4, cg = 4 * np + q;
    h8 wh[2], wl[2];
    f32x4 ws[2], wt[2];
#pragma unroll
    for (int n = 0; n < 2; n++) {
        const int ch0 = dg_ch0(np, q, n);
        const _Float16* wf = (const _Float16*)(W + F16_C0) + (size_t)(dg_wfrag(np, lane) + n * DG_WFRAG_N) * 8;
        wh[n] = *(const h8*)wf;
        wl[n] = *(const h8*)(wf + 8 * 64 * 8);
        ws[n] = *(const f32x4*)(W + C0_S + ch0);
        wt[n] = *(const f32x4*)(W + C0_T + ch0);
    }
    _Float16* in = (_Float16*)(lds + K::IN);
    // every node's root x0 values first (one round of latency for the chunk), then the MFMAs
    h8 rxh[K::C], rxl[K::C];
    f32x4 rxp[OVERLAY ? K::C : 1][2];  // OVERLAY: the parent's patch row where it covers the position
    bool inp[OVERLAY ? K::C : 1];
#pragma unroll
    for (int g = 0; g < K::C; g++) {
        const DgUnit& u = U[g < ng ? g : 0];
        const int cr = u.cell / BN, cc = u.cell - (u.cell / BN) * BN;
        const int r0 = cr > 0 ? cr - 1 : 0, r1 = cr < BN - 1 ? cr + 1 : BN - 1;
        const int c0 = cc > 0 ? cc - 1 : 0, c1 = cc < BN - 1 ? cc + 1 : BN - 1, wr = c1 - c0 + 1;
        const bool rowok = li < (r1 - r0 + 1) * wr;
        const int pr = rowok ? r0 + li / wr : cr, pc = rowok ? c0 + li % wr : cc, pos = pr * BN + pc;
        const _Float16* rp = u.gm + (cg * 256 + pos) * 8;
        rxh[g] = gld<h8>(rp);
        rxl[g] = gld<h8>(rp + PV_MAP_PLANE);
        if (OVERLAY) {
            const int pcell = u.pcell, oy = pr - pcell / BN, ox = pc - (pcell - (pcell / BN) * BN);
            inp[g] = iabs(oy) <= 1 && iabs(ox) <= 1;
            rxp[g][0] = rxp[g][1] = zero4();
            if (inp[g]) {  // (a written row: the position is on the board and in the parent's square)
                const float* pp = u.patch + (PATCH_POS[0] + (oy + 1) * 3 + (ox + 1)) * CH + 8 * cg;
                rxp[g][0] = gld<f32x4>(pp);
                rxp[g][1] = gld<f32x4>(pp + 4);
            }
        }
    }
#pragma unroll
    for (int g = 0; g < K::C; g++) {
        if (g >= ng) break;
        const h8 a = *(const h8*)(col + g * 512 + li * 32 + 8 * q);
        const DgUnit& u = U[g];
        const int cr = u.cell / BN, cc = u.cell - (u.cell / BN) * BN;
        const int r0 = cr > 0 ? cr - 1 : 0, r1 = cr < BN - 1 ? cr + 1 : BN - 1;
        const int c0 = cc > 0 ? cc - 1 : 0, c1 = cc < BN - 1 ? cc + 1 : BN - 1, wr = c1 - c0 + 1;
        const bool rowok = li < (r1 - r0 + 1) * wr;
        const int pr = rowok ? r0 + li / wr : cr, pc = rowok ? c0 + li % wr : cc;
        const int idx = (pr - cr + 1) * 3 + (pc - cc + 1);
        f32x4 y[2], d[2];
#pragma unroll
        for (int n = 0; n < 2; n++) {
            f32x4 acc = zero4();
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wh[n], a, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(wl[n], a, acc, 0, 0, 0);
#pragma unroll
            for (int r = 0; r < 4; r++) {
                float t = __builtin_fmaf(acc[r], ws[n][r], wt[n][r]);
                t = t > 0.f ? t : 0.f;
                y[n][r] = t;
                float ref = (float)rxh[g][4 * n + r] + (float)rxl[g][4 * n + r];  // the root's x0
                if (OVERLAY) ref = inp[g] ? rxp[g][n][r] : ref;
                d[n][r] = t - ref;
            }
        }
        if (rowok) {
            const H8x2 dd = split_hl(d);
            put_hl_lds(in + (cg * NPOS + g * 9 + idx) * 8, 16 * NPOS * 8, dd);
            put_hl(u.own + u.sq[0] + (cg * 9 + idx) * 8, 16 * 9 * 8, dd);
            if (!OVERLAY && u.patch) put_f8(u.patch + (PATCH_POS[0] + idx) * CH + 8 * cg, y);
        }
    }
}

// ------------------------------------------------------------------ one pass
// the row VGPRs of the lane for every tile, then the k-loop at the smallest tile-count
// instantiation that covers the pass's tiles
template <int L>
__device__ __forceinline__ void dg_pass(const char* lds, const uint32_t* rt, const uint32_t* mk,
                                        const float* __restrict__ W, int np, int lane, f32x4 (&acc)[2][K::NMAX], int nt) {
    constexpr int RIN = L + 1, RO = L + 2, S = dg_s(L), SS = dg_ss(L);
    const int li = lane & 15;
    uint32_t ri[K::NMAX];
#pragma unroll
    for (int m = 0; m < K::NMAX; m++) {
        const uint32_t e = rt[m * 16 + li];
        const int gi = e & 15, dy = (int)((e >> 4) & 15) - RO, dx = (int)((e >> 8) & 15) - RO;
        const int base = gi * SS + (dy + RIN) * S + (dx + RIN) + 32;
        ri[m] = (e >> 21) & 1u ? ((uint32_t)base & 0xffffu) | (((e >> 12) & 0x1ffu) << 16) : 0u;
    }
#pragma unroll
    for (int n = 0; n < 2; n++)
#pragma unroll
        for (int m = 0; m < K::NMAX; m++) acc[n][m] = zero4();
    const _Float16* Wf = (const _Float16*)(W + F16_RES0 + L * F16_STRIDE);
    // the tile count rounded up to a multiple of 4: the padding tiles (no rows, no taps)
    // still cost their fragment reads
#if GZ_DG_NTE
    // instantiated per even tile count up to the layer's most: a padding tile costs
    // its fragment reads and their wait
    constexpr int MT = (dgk_g(L) * dg_so(L) * dg_so(L) + 15) / 16, MTE = (MT + 1) & ~1;
    static_assert(MTE <= K::NMAX, "tiles");
    const int nte = (nt + 1) & ~1;
    if (nte <= 2)
        dg_kloop<2, L>(lds, ri, mk, Wf, 2 * np, lane, acc);
    else if (nte == 4)
        dg_kloop<4, L>(lds, ri, mk, Wf, 2 * np, lane, acc);
    else if (nte == 6 || MTE <= 6)
        dg_kloop<6 < MTE ? 6 : MTE, L>(lds, ri, mk, Wf, 2 * np, lane, acc);
    else if (nte == 8 || MTE <= 8)
        dg_kloop<8 < MTE ? 8 : MTE, L>(lds, ri, mk, Wf, 2 * np, lane, acc);
    else if (nte == 10 || MTE <= 10)
        dg_kloop<10 < MTE ? 10 : MTE, L>(lds, ri, mk, Wf, 2 * np, lane, acc);
    else
        dg_kloop<MTE, L>(lds, ri, mk, Wf, 2 * np, lane, acc);
#else
    if (nt <= 4)
        dg_kloop<4, L>(lds, ri, mk, Wf, 2 * np, lane, acc);
    else if (nt <= 8)
        dg_kloop<8, L>(lds, ri, mk, Wf, 2 * np, lane, acc);
    else
        dg_kloop<K::NMAX, L>(lds, ri, mk, Wf, 2 * np, lane, acc);
#endif
}

// pass p of a chunk of ng nodes: its layer L, first node u0 and node count g (0: empty)
__device__ __forceinline__ void dg_pass_of(int p, int ng, int& L, int& u0, int& g) {
    if (p < 3) {  // (K::pass_of inverted)
        L = p == 0 ? 0 : 1;
        u0 = p == 0 ? 0 : (p - 1) * 3;
    } else {
        const int k = (p - 3) / 3, r = p - 3 - 3 * k;
        L = r == 0 ? 2 : 3;
        u0 = 2 * k + (r == 2 ? 1 : 0);
    }
    g = ng - u0 < K::g(L) ? ng - u0 : K::g(L);
    if (L == 0) u0 = 0, g = ng;
}

// OVERLAY = false: the root children (list: t.children), each a delta of its root.
// OVERLAY = true: the grandchildren (list: t.grand, a parent's adjacent), each a delta of
// its parent: the same passes with the parent's values (its patch inside its changed
// squares, the root's elsewhere) in place of the root's, its record on the parent's.
template <bool OVERLAY>
__global__ __launch_bounds__(NTD, K::WPS) void pv_dg_kernel(DgArgs A, _Float16* __restrict__ scratch,
                                                           const int32_t* __restrict__ list,
                                                           const int32_t* __restrict__ list_count) {
    __shared__ __attribute__((aligned(16))) char lds[K::LDS];
    DgUnit* const U = (DgUnit*)(lds + K::U);
    const int count = *list_count;
    // XCD-aware interleave: XCD x = blockIdx % 8 takes a contiguous eighth of the list
    // and its workgroups take its chunks in turn, so one XCD works on a few roots at a
    // time (their maps and pre-ReLU values stay in that XCD's L2)
    const int nx = gridDim.x >= 8 ? 8 : 1;
    const int xcd = blockIdx.x % nx, per = gridDim.x / nx, k = blockIdx.x / nx;
    if (k >= per) return;
    const int xchunk = (count + nx - 1) / nx;
    // The XCD's chunks are taken from its queue head in turn (a workgroup that finishes
    // early takes more: no static share, no tail); once the XCD's eighth is exhausted its
    // workgroups help the other XCDs (q = xcd + 1, ...), so no XCD finishes last alone.
    // Thread 0 holds the claim (queue q, offset), made one chunk ahead so that the
    // atomic's latency is hidden, and publishes each chunk's (first entry, end) in LDS.
    int q = 0, claim = 0;
    if (threadIdx.x == 0) claim = atomicAdd(A.queue + xcd, K::C);
    _Float16* myscr = scratch + (size_t)blockIdx.x * SCR_HALVES;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6), np = wave;
    const float* W = A.W;
    for (int i = tid; i < K::NPASS * K::NKEY; i += NTD) ((uint32_t*)(lds + K::HIST))[i] = 0u;
    {  // the epilogues' per-channel constants: BN scales of y1, x1, y2, x2, the 1x1 heads' weights and biases
        float* cst = (float*)(lds + K::CST);
        for (int i = tid; i < K::CST_FLOATS; i += NTD) {
            float v;
            if (i < 512) v = W[RES0 + (i >> 7) * RES_STRIDE + RES_S + (i & 127)];
            else if (i < 768) v = W[P_W + (i - 512)];
            else if (i < 896) v = W[V_W + (i - 768)];
            else v = i == 896 ? W[P_B] : (i == 897 ? W[P_B + 1] : (i == 898 ? W[V_B] : 0.f));
            cst[i] = v;
        }
    }
    typename std::conditional<OVERLAY, PhaseStamp<nullptr>, DgStamp>::type st;
    for (;;) {
        __syncthreads();  // the previous chunk's readers of U, hpart, the tables and POS are done
        if (threadIdx.x == 0) {
            int pb = count, pe = count;  // (none left: the loop ends)
            for (;;) {
                const int qx = (xcd + q) % nx, xb = qx * xchunk, xe = xb + xchunk < count ? xb + xchunk : count;
                if (xb + claim < xe) {
                    pb = xb + claim, pe = xe;
                    claim = atomicAdd(A.queue + qx, K::C);
                    break;
                }
                if (++q == nx) break;
                claim = atomicAdd(A.queue + (xcd + q) % nx, K::C);
            }
            ((int*)(lds + K::POS))[0] = pb;
            ((int*)(lds + K::POS))[1] = pe;
        }
        __syncthreads();
        const int pos = ((const int*)(lds + K::POS))[0], xe = ((const int*)(lds + K::POS))[1];
        if (pos >= xe) break;
        const int ng = xe - pos < K::C ? xe - pos : K::C;
        if (wave == 0 && lane < ng) {
            const int b = list[pos + lane];
            DgUnit u;
            const int ci = A.cinfo[b];
            const int o = (ci >> 8) & 0x3fffff;
            u.gm = A.maps + (size_t)o * PV_MAP_HALVES;
            u.pre = A.pres + (size_t)o * 4 * PV_PRE_FLOATS;
            u.own = myscr;
            u.sq[0] = scr_sq(0, lane);
            u.sq[1] = scr_sq(1, lane);
            u.sq[2] = scr_sq(2, lane);
            u.sq[3] = scr_sq(3, lane);
            u.leaf = b;
            u.base = A.meta[b];
            u.cell = ci & 0xff;
            if (OVERLAY) {  // the parent (u.base): a root child with a patch slot (tree_lists_kernel)
                u.patch = A.patches + (size_t)A.pslot[u.base] * PATCH_FLOATS;
                u.pcell = A.cinfo[u.base] & 0xff;
            } else {
                const int ps = A.pslot[b];
                u.patch = ps >= 0 ? A.patches + (size_t)ps * PATCH_FLOATS : nullptr;
                u.pcell = 0;
            }
#pragma unroll
            for (int w = 0; w < 16; w++) u.board[w] = A.boards[(size_t)b * 16 + w];
            U[lane] = u;
        }
        __syncthreads();
        {  // conv0 and D(x0): the y1 pass's image (zero past the nodes' squares); every
           // pass's row table
            int t = tid;
            asm volatile("" : "+v"(t));
            dg_col((_Float16*)(lds + K::COL), U, ng, t);
            constexpr int NPOS0 = K::npos(0);
            const int z0 = ng * 9;
            for (int e = t; e < 32 * (NPOS0 - z0); e += NTD) {
                const int pc = e / (NPOS0 - z0), idx = z0 + e % (NPOS0 - z0);
                *(uint4*)(lds + K::IN + (pc * NPOS0 + idx) * 16) = make_uint4(0u, 0u, 0u, 0u);
            }
            __syncthreads();
            const float* Wp = W;
            asm volatile("" : "+s"(Wp));
            dg_conv0<OVERLAY>(lds, (const _Float16*)(lds + K::COL), U, ng, Wp, np, t & 63);
            dg_rows_all(lds, U, ng, t);
            __syncthreads();  // the y1 image, the row tables and tap masks
#ifdef GZ_DG_CHK
            // every table entry below its pass's row count names a node of that pass
            for (int e = tid; e < K::NPASS * K::ROWS; e += NTD) {
                const int pp = e / K::ROWS;
                int L_, u0_, g_;
                dg_pass_of(pp, ng, L_, u0_, g_);
                const uint32_t tot = ((const uint32_t*)(lds + K::MASK))[pp * 16 + 9];
                const uint32_t en = ((const uint32_t*)(lds + K::ROWT))[e];
                if ((uint32_t)(e % K::ROWS) < tot && (!((en >> 21) & 1u) || (int)(en & 15) >= g_))
                    atomicAdd(&gz_dg_chk[8], 1ull);
                if ((uint32_t)(e % K::ROWS) >= tot && en != 0u) atomicAdd(&gz_dg_chk[9], 1ull);
            }
            if (tid < K::C && (U[tid].cell < 0 || U[tid].cell >= 225) && tid < ng) atomicAdd(&gz_dg_chk[10], 1ull);
#endif
        }
        st(0);
#ifdef GZ_PVDG_STAMPS
        if (!OVERLAY && blockIdx.x == 0 && threadIdx.x == 0) atomicAdd(&gz_pvdg_stamps_n[0], (unsigned long long)ng);
#endif
        for (int p = 0; p < K::NPASS; p++) {
            int L, u0, g;
            dg_pass_of(p, ng, L, u0, g);
            if (g <= 0) continue;
            const uint32_t* rt = (const uint32_t*)(lds + K::ROWT) + p * K::ROWS;
            const uint32_t* mk = (const uint32_t*)(lds + K::MASK) + p * 16;
            const int nrows = (int)mk[9], nt = (nrows + 15) >> 4;
            if (A.tiles && tid == 0) atomicAdd(A.tiles, (int)mk[10]);
            const float* Wp = W;
            int t = tid;
            asm volatile("" : "+s"(Wp), "+v"(t));
#ifdef GZ_DG_CHK
            for (int e = tid; e < K::ROWS; e += NTD) {
                const uint32_t en = rt[e];
                if ((uint32_t)e < (uint32_t)nrows && (!((en >> 21) & 1u) || (int)(en & 15) >= g))
                    atomicAdd(&gz_dg_chk[11 + (L > 1 ? 1 : 0)], 1ull);
            }
#endif
            f32x4 acc[2][K::NMAX];
            if (L == 0) dg_pass<0>(lds, rt, mk, Wp, np, t & 63, acc, nt);
            else if (L == 1) dg_pass<1>(lds, rt, mk, Wp, np, t & 63, acc, nt);
            else if (L == 2) dg_pass<2>(lds, rt, mk, Wp, np, t & 63, acc, nt);
            else dg_pass<3>(lds, rt, mk, Wp, np, t & 63, acc, nt);
            st(2 + L);
            __syncthreads();  // every wave is past the k-loop: the image is free
            st(6);
            // the next non-empty pass (its fill follows the epilogue: issued under it, the
            // epilogue's loads would wait for the fill's LDS-DMA -- measured slower)
            int q = p + 1, L2 = 0, v0 = 0, g2 = 0;
            for (; q < K::NPASS; q++) {
                dg_pass_of(q, ng, L2, v0, g2);
                if (g2 > 0) break;
            }
            const bool more = q < K::NPASS;
            // When the next pass is the next layer of this pass's first nodes (y1 -> x1(0..2),
            // y2(2k, 2k+1) -> x2(2k)), those nodes' D squares go straight into the next
            // pass's LDS image (dg_fill's layout) instead of the scratch: no store, no fill,
            // no drain; the pass's other nodes go through the scratch as before.  (The
            // epilogue's scattered stores of the D squares are 15 % of the kernel.)
            const int ldsg = more && L2 == L + 1 && v0 == u0 && (L == 0 || L == 2) ? g2 : 0;
            const bool to_lds = ldsg > 0;
            if (L == 0) dg_epilogue<0, OVERLAY>(lds, U + u0, rt, np, t & 63, acc, nt, ldsg);
            else if (L == 1) dg_epilogue<1, OVERLAY>(lds, U + u0, rt, np, t & 63, acc, nt, 0);
            else if (L == 2) dg_epilogue<2, OVERLAY>(lds, U + u0, rt, np, t & 63, acc, nt, ldsg);
            else dg_epilogue<3, OVERLAY>(lds, U + u0, rt, np, t & 63, acc, nt, 0);
            if (to_lds) {  // the image's zero slots past the nodes' squares (dg_fill writes them)
                const int NPN = L == 0 ? K::npos(1) : K::npos(3), z0 = ldsg * (L == 0 ? dg_ss(1) : dg_ss(3));
                for (int e = t; e < 32 * (NPN - z0); e += NTD) {
                    const int pc = e / (NPN - z0), idx = z0 + e % (NPN - z0);
                    *(uint4*)(lds + K::IN + (pc * NPN + idx) * 16) = make_uint4(0u, 0u, 0u, 0u);
                }
            }
            st(7 + L);
            // vmcnt counts loads, stores and LDS-DMA together in issue order, so each wait
            // below also waits for every older store.  The next pass's fill reads, by
            // LDS-DMA, squares that older passes stored -- and this pass's only when it is
            // the next layer over some of the same nodes (y1 -> the first x1 pass): then
            // every wave's stores complete before a barrier first.  x2: the barrier
            // publishes hpart for the record.
            const bool reads_mine = more && !to_lds && L2 == L + 1 && v0 < u0 + g && u0 < v0 + g2;
            if (reads_mine) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            if (reads_mine || L == 3) __syncthreads();
            st(11);
            // the fill goes out first; an x2 pass's record (the root's record loaded, the
            // node's written) follows, its loads in flight with the fill's
            if (more && !to_lds) {
                if (L2 == 1) dg_fill<1>(lds, U + v0, g2, t);
                else if (L2 == 2) dg_fill<2>(lds, U + v0, g2, t);
                else if (L2 == 3) dg_fill<3>(lds, U + v0, g2, t);
            }
            if (L == 3) {  // (the root's record entries loaded here: held across the epilogue they were spilled)
                float rec[REC_K];
                dg_record_load(U[u0], A.hbuf, rec, t);
                dg_record(U[u0], 0, (const float*)(lds + K::CST) + 896, A.hbuf, (const float*)(lds + K::HP), rec, t);
                // every thread stores >= 2 record entries after the fill: all but the 2
                // youngest operations done = the fill landed
                asm volatile("s_waitcnt vmcnt(2)" ::: "memory");
            } else {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            }
            st(12);
            __syncthreads();  // the image has landed (and hpart is free again)
            st(13);
        }
    }
}

}  // namespace

// the root children (t.children, t.ctr[CTR_CHILDREN] entries) of gz_pv_forward_tree
// through pv_dg_kernel, then the grandchildren (t.grand, t.ctr[CTR_GRAND] entries, parent
// order) through its overlay form; t.scratch: PV_SCRATCH_AREAS areas per CU (grid = CUs)
int gz_internal_tree_delta(const TreeWs& t, const float* d_weights, const uint32_t* d_boards, const int32_t* d_meta,
                           int grid, void* stream) {
    DgArgs A{t.cinfo, d_weights, d_boards, d_meta, t.pslot, t.maps, t.pres, t.patches, t.hbuf,
             t.ctr + CTR_TILES, t.ctr + CTR_DG_QUEUE};
    // K::WPS workgroups per grid entry (CU), K::C patch-sized scratch areas each
    static_assert(K::WPS * SCR_HALVES <= PV_SCRATCH_AREAS * PV_SCRATCH_AREA_HALVES, "scratch");
#ifdef GZ_PVDG_STAMPS
    // stamp builds: GZ_PVDG_WPS=1 runs one workgroup per CU (the k-loop without a co-resident one)
    static const int wps = std::getenv("GZ_PVDG_WPS") && std::getenv("GZ_PVDG_WPS")[0] == '1' ? 1 : K::WPS;
#else
    constexpr int wps = K::WPS;
#endif
#ifdef GZ_DG_CHK
    {
        const char* lo = (const char*)t.hbuf;
        const char* hi = (const char*)(t.scratch + (size_t)grid * PV_SCRATCH_AREAS * PV_SCRATCH_AREA_HALVES);
        hipMemcpyToSymbolAsync(HIP_SYMBOL(gz_dg_lo), &lo, sizeof(lo), 0, hipMemcpyHostToDevice, (hipStream_t)stream);
        hipMemcpyToSymbolAsync(HIP_SYMBOL(gz_dg_hi), &hi, sizeof(hi), 0, hipMemcpyHostToDevice, (hipStream_t)stream);
    }
#endif
    pv_dg_kernel<false><<<grid * wps, NTD, 0, (hipStream_t)stream>>>(A, t.scratch, t.children, t.ctr + CTR_CHILDREN);
    // the grandchildren: their parents' patches and records are written; tile-taps to the
    // grandchildren's counter, a queue of their own
    A.tiles = t.ctr + CTR_TILES + 1;
    A.queue = t.ctr + CTR_GRAND_QUEUE;
    pv_dg_kernel<true><<<grid * wps, NTD, 0, (hipStream_t)stream>>>(A, t.scratch, t.grand, t.ctr + CTR_GRAND);
    return gz_check_launch("tree delta");
}

#ifdef GZ_PVDG_STAMPS
// phase stamps of workgroup 0 (-DGZ_PVDG_STAMPS builds, tools/pvinc_bench.py): out[0..15]
// ticks per phase, out[16] nodes
extern "C" int gz_pvdg_stamps_read(unsigned long long* out, int reset) {
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(gz_pvdg_stamps), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (hipMemcpyFromSymbol(out + 16, HIP_SYMBOL(gz_pvdg_stamps_n), sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) {
        unsigned long long z[16] = {0};
        if (hipMemcpyToSymbol(HIP_SYMBOL(gz_pvdg_stamps), z, sizeof(z)) != hipSuccess) return -1;
        if (hipMemcpyToSymbol(HIP_SYMBOL(gz_pvdg_stamps_n), z, sizeof(z[0])) != hipSuccess) return -1;
    }
    return 0;
}
#endif

#ifdef GZ_DG_CHK
// out-of-workspace global accesses per code (loads, stores, fills, record reads, record writes)
extern "C" int gz_pvdg_chk_read(unsigned long long* out) {
    if (hipDeviceSynchronize() != hipSuccess) return -1;
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(gz_dg_chk), 16 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
#endif
