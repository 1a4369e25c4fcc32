// Stand-alone reader of snprelate_amd/csrc/proj_grid.h (test_cpu_proj_grid.py builds it with the host compiler and the address and
// undefined-behaviour sanitizers and runs it): for every input line "snp N n_snp k" or "samp N n_snp k" it prints that line followed
// by "gx gy split per", the launch geometry of the projection kernels for that shape.  A line it cannot read ends it with status 1.
#include <cstdio>
#include <cstring>

#include "proj_grid.h"

int main()
{
    char side[16];
    long long N, n_snp;
    int k;
    for (;;) {
        const int got = std::scanf("%15s %lld %lld %d", side, &N, &n_snp, &k);
        if (got == EOF) return 0;
        const bool snp = !std::strcmp(side, "snp");
        if (got != 4 || (!snp && std::strcmp(side, "samp")) || N <= 0 || n_snp <= 0 || k <= 0) {
            std::fprintf(stderr, "proj_grid_check: bad input line\n");
            return 1;
        }
        const snpgpu::ProjGrid g = snp ? snpgpu::proj_snp_grid(N, n_snp, k) : snpgpu::proj_samp_grid(N, n_snp, k);
        std::printf("%s %lld %lld %d %lld %lld %lld %lld\n", side, N, n_snp, k, (long long)g.gx, (long long)g.gy, (long long)g.split,
                    (long long)g.per);
    }
}
