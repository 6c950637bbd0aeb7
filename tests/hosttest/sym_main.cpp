// csrc/gz_sym.h on the host (tests/test_sym_hostcheck_cpu.py builds this with
// -fsanitize=address,undefined): sym_src against sym_dst for all 8 x 225 cells, boards that
// touch all four edges transformed and mapped back through the two, and sym_of of the
// known-answer rows.  Prints "ok", then one line "sym <seed> <what> <t>" per row; a
// failed check prints "FAIL ..." and exits 1.
#include <cstdio>
#include <cstring>

#include "../../alphazero-gomoku_amd/csrc/gz_sym.h"

using namespace gz;

static void set_cell(uint32_t* row, int cell, int colour) {
    const int b = cell_to_bit(cell);
    row[(colour == 2 ? 8 : 0) + (b >> 5)] |= 1u << (b & 31);
}

static int get_cell(const uint32_t* row, int cell) {
    const int b = cell_to_bit(cell);
    if ((row[b >> 5] >> (b & 31)) & 1u) return 1;
    if ((row[8 + (b >> 5)] >> (b & 31)) & 1u) return 2;
    return 0;
}

// y = T_t(x) the way the kernel builds it: output cell c reads x[sym_src(t, c)]
static void transform(const uint32_t* x, int t, uint32_t* y) {
    std::memset(y, 0, 16 * sizeof(uint32_t));
    for (int c = 0; c < GZ_CELLS; c++) {
        const int v = get_cell(x, sym_src(t, c));
        if (v) set_cell(y, c, v);
    }
}

int main() {
    for (int t = 0; t < 8; t++) {
        bool seen[GZ_CELLS] = {};
        for (int c = 0; c < GZ_CELLS; c++) {
            const int s = sym_src(t, c);
            if (s < 0 || s >= GZ_CELLS || seen[s]) return std::printf("FAIL src %d %d\n", t, c), 1;
            seen[s] = true;
            if (sym_dst(t, s) != c) return std::printf("FAIL dst %d %d\n", t, c), 1;
            if (t == 0 && s != c) return std::printf("FAIL identity %d\n", c), 1;
        }
    }
    // two boards that touch all four edges: the corners and edge midpoints, and a diagonal
    // band with both colours
    uint32_t boards[2][16] = {};
    const int edge[8] = {0, 7, 14, 15 * 7, 15 * 7 + 14, 15 * 14, 15 * 14 + 7, 224};
    for (int i = 0; i < 8; i++) set_cell(boards[0], edge[i], 1 + (i & 1));
    for (int r = 0; r < GZ_N; r++) {
        set_cell(boards[1], r * GZ_N + r, 1);
        if (r + 1 < GZ_N) set_cell(boards[1], r * GZ_N + r + 1, 2);
    }
    set_cell(boards[1], 14, 2);
    set_cell(boards[1], 14 * GZ_N, 1);
    for (int b = 0; b < 2; b++)
        for (int t = 0; t < 8; t++) {
            uint32_t y[16], back[16] = {};
            transform(boards[b], t, y);
            for (int w = 0; w < 16; w++)
                if (y[w] & ~valid_word(w & 7)) return std::printf("FAIL guard %d %d\n", b, t), 1;
            for (int c = 0; c < GZ_CELLS; c++) {  // x[c] = y[sym_dst(t, c)]
                const int v = get_cell(y, sym_dst(t, c));
                if (v) set_cell(back, c, v);
            }
            if (std::memcmp(back, boards[b], sizeof(back)) != 0) return std::printf("FAIL round trip %d %d\n", b, t), 1;
        }
    std::printf("ok\n");
    uint32_t row[16] = {};
    std::printf("sym 3 empty %d\n", sym_of(3, row));
    std::printf("sym 0 empty %d\n", sym_of(0, row));
    for (int c = 0; c < 16; c++) {
        std::memset(row, 0, sizeof(row));
        set_cell(row, c, 1);
        std::printf("sym 3 black%d %d\n", c, sym_of(3, row));
    }
    return 0;
}
