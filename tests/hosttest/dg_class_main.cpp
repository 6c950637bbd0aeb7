// Prints pv_dg_kernel's row-class order (csrc/gz_dgclass.h dg_class_rank) on the host:
// one line "ty tx rank" per valid pair of tap sets (tests/test_dg_class_order_cpu.py).
#include <cstdio>

#include "../../alphazero-gomoku_amd/csrc/gz_dgclass.h"

int main() {
    const int sets[6] = {1, 3, 7, 6, 4, 2};  // {-1}, {-1,0}, {-1,0,1}, {0,1}, {1}, {0}
    for (int a = 0; a < 6; a++)
        for (int b = 0; b < 6; b++) std::printf("%d %d %d\n", sets[a], sets[b], dg_class_rank(sets[a], sets[b]));
    return 0;
}
