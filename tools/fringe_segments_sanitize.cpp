// Stand-alone host check of the segment plan of a merged pair launch (seg_plan / seg_block, csrc/fringe_mfma_common.h) under
// ASan + UBSan: enumerates every block of a set of shapes in both directions and checks that each (segment, f, t, split)
// occurs once and that the panel / tile ranges tile every segment.
//   hipcc -O1 -g -std=c++17 --offload-arch=gfx950 -x hip -Xarch_host -fsanitize=address,undefined -fno-gpu-sanitize \
//         tools/fringe_segments_sanitize.cpp -o fringe_segments_sanitize && ./fringe_segments_sanitize
#include "../bayeslim_amd/csrc/fringe_mfma_common.h"
#include <cstdio>
#include <vector>

using namespace rime;

static bool check(bool backward, int Nt, int Nf, const std::vector<int>& Ps)
{
    SegPlan p;
    if (!seg_plan(backward, true, Nt, Nf, Ps.data(), (int)Ps.size(), p)) return false;
    std::vector<std::vector<int>> seen(Ps.size());
    std::vector<long> covered(Ps.size(), 0);
    for (size_t k = 0; k < Ps.size(); ++k) seen[k].assign((size_t)Nt * Nf * p.S[k], 0);
    for (long b = 0; b < p.grid; ++b) {
        const SegBlock r = seg_block(p, Nf, Ps.data(), backward, b);
        if (r.seg < 0 || r.seg >= (int)Ps.size() || r.f < 0 || r.f >= Nf || r.t < 0 || r.t >= Nt || r.split < 0 || r.split >= p.S[r.seg]) return false;
        if (r.begin != r.split * p.per[r.seg] || r.end <= r.begin || r.end > Ps[r.seg] / 32) return false;
        int& s = seen[r.seg][((size_t)r.t * p.S[r.seg] + r.split) * Nf + r.f];
        if (s++) return false;
        if (r.f == 0 && r.t == 0) covered[r.seg] += r.end - r.begin;
    }
    for (size_t k = 0; k < Ps.size(); ++k) {
        if (covered[k] != Ps[k] / 32) return false;
        for (int s : seen[k]) if (s != 1) return false;
    }
    return true;
}

int main()
{
    const std::vector<std::vector<int>> sets = {{128, 64}, {64, 64, 128}, {16448, 64}, {128, 2112}, {64}, {64, 64, 64, 64},
                                                {98304, 10048}, {10048, 98304}, {98304}, {1 << 21, 64, 4096}};
    const int shapes[][2] = {{2, 3}, {1, 1}, {8, 256}, {3, 1000}};
    long checked = 0;
    for (const auto& Ps : sets) for (const auto& sh : shapes) for (int backward = 0; backward < 2; ++backward) {
        if (!check(backward != 0, sh[0], sh[1], Ps)) { printf("FAIL Nt %d Nf %d set of %zu backward %d\n", sh[0], sh[1], Ps.size(), backward); return 1; }
        ++checked;
    }
    SegPlan f, b;
    const int c4[] = {98304, 10048};
    seg_plan(false, true, 8, 256, c4, 2, f);
    seg_plan(true, true, 8, 256, c4, 2, b);
    printf("%ld plans ok; C4 forward grid %ld slabs %ld, backward grid %ld (S %d + %d)\n", checked, f.grid, f.slabs, b.grid, b.S[0], b.S[1]);
    const int bad[] = {96};
    return !(f.grid == 2048 * 7 && f.slabs == 7 && b.grid == 2048 * 4 && b.S[0] == 3 && b.S[1] == 1 && !seg_plan(false, true, 2, 3, bad, 1, f)
             && !seg_plan(false, true, 2, 3, c4, 5, f));
}
