// Host program of tests/test_layouts_host.py.  No GPU, no oracle: csrc/fk_layouts.h is plain host arithmetic.
//   stdin, one layout per line:
//     game_stats S rounds_bins margin_bins spill_capacity
//     rare S second_bins
//     fingerprints game_seed_bytes shuffle_seed_bytes
//     root_params n_k S joint
//   stdout, one line each: the struct's members in their order of declaration, then what its functions give (game_stats: spill_at, bytes)
#include <cstdio>
#include <cstring>

#include "../../farkle_ii_amd/csrc/fk_layouts.h"

int main() {
    char kind[32];
    long long a, b, c, d;
    while (scanf("%31s", kind) == 1) {
        if (!strcmp(kind, "game_stats") && scanf("%lld %lld %lld %lld", &a, &b, &c, &d) == 4) {
            const fkl::GameStatsOut g((size_t)a, (size_t)b, (size_t)c);
            printf("%zu %zu %zu %zu %zu %zu %zu %zu %zu %zu %zu\n", g.s_counts, g.s_rounds, g.s_runner, g.s_spread, g.g_counts, g.g_rounds, g.g_runner,
                   g.spill_count, g.n_u64, g.spill_at(), g.bytes((int64_t)d));
        } else if (!strcmp(kind, "rare") && scanf("%lld %lld", &a, &b) == 2) {
            const fkl::RareOut r((size_t)a, (size_t)b);
            printf("%zu %zu %zu %zu\n", r.s_second, r.g_second, r.total, r.n_u64);
        } else if (!strcmp(kind, "fingerprints") && scanf("%lld %lld", &a, &b) == 2) {
            const fkl::Fingerprints f((size_t)a, (size_t)b);
            printf("%zu %zu %zu\n", f.game_at, f.shuffle_at, f.bytes);
        } else if (!strcmp(kind, "root_params") && scanf("%lld %lld %lld", &a, &b, &c) == 3) {
            const fkl::RootParams p((size_t)a, (size_t)b, c != 0);
            printf("%zu %zu %zu %zu %zu %zu\n", p.weights, p.observed, p.expected, p.observed_across, p.expected_across, p.n);
        } else {
            return 1;
        }
    }
    return 0;
}
