// Stand-alone host check of the backward pixel-split plans (csrc/fringe_mfma_common.h) under ASan + UBSan: sweeps shapes
// up to the largest the block entries accept and checks that the splits cover every tile exactly once.
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -x hip -Xarch_host -fsanitize=address,undefined -fno-gpu-sanitize \
//         tools/pair_split_sanitize.cpp -o pair_split_sanitize && ./pair_split_sanitize
#include "../bayeslim_amd/csrc/fringe_mfma_common.h"
#include <cstdio>

int main()
{
    using namespace rime;
    const int nts[] = {1, 2, 8, 64, 65535}, nfs[] = {1, 3, 256, 4096, 1 << 20};
    const int ps[] = {64, 2112, 10048, 49152, 98304, 98240, 1 << 24, 2147483584};
    long checked = 0;
    for (int Nt : nts) for (int Nf : nfs) for (int P : ps) {
        const int ntile = P / 32;
        const PixelSplit b = bwd_split_plan(Nt, Nf, P), p = pair_bwd_split_plan(Nt, Nf, P);
        for (const PixelSplit& s : {b, p})
            if (s.S < 1 || s.per < 1 || (long)(s.S - 1) * s.per >= ntile || (long)s.S * s.per < ntile) {
                printf("FAIL Nt %d Nf %d P %d: S %d per %d\n", Nt, Nf, P, s.S, s.per);
                return 1;
            }
        if (p.S > b.S || p.per > 1024 || (p.per != b.per && (long)Nt * Nf * p.S < PAIR_BWD_MIN_GRID)) {
            printf("FAIL Nt %d Nf %d P %d: pair S %d per %d, base S %d per %d\n", Nt, Nf, P, p.S, p.per, b.S, b.per);
            return 1;
        }
        ++checked;
    }
    const PixelSplit c4 = pair_bwd_split_plan(8, 256, 98304), ps4 = pair_bwd_split_plan(8, 256, 10048);
    printf("%ld shapes ok; C4 diffuse S %d per %d, point sources S %d per %d\n", checked, c4.S, c4.per, ps4.S, ps4.per);
    return !(c4.S == 3 && c4.per == 1024 && ps4.S == 2 && ps4.per == 256);
}
