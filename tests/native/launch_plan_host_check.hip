// Host program of the launch-plan fixture (tests/golden/launch_plan.json).  No GPU, no oracle: fk_plan.h is plain host C++.
//   stdin, one call per line:  mode cus k S single_batch target_score max_waves blocks_per_cu block lean state_store hot_cold use_lds_tally
//                              (mode 0 tournament, 1 game list, 2 batched H2H; the options as fk_set_option stores them)
//   stdout, one plan per line: block grid lds lds_tally lean gs blk hc shape      or "none" when no instance fits
//   The shape is the planned row's kernel template as tests/kernel_instances.py spells it, {m} in the place of the MIXED argument.
#include <cstdio>

#include "../../farkle_ii_amd/csrc/fk_kernels.h" // the constants the planner takes from the kernels' headers
#include "../../farkle_ii_amd/csrc/fk_plan.h"

int main() {
    int mode, cus, k, single, target;
    long long S;
    PlanKnobs kn;
    while (scanf("%d %d %d %lld %d %d %d %d %d %d %d %d %d", &mode, &cus, &k, &S, &single, &target, &kn.max_waves, &kn.blocks_per_cu, &kn.block,
                 &kn.lean, &kn.gs, &kn.hc, &kn.use_lds_tally) == 13) {
        kn.cus = cus;
        const LaunchPlan p = plan_play(kn, (PlanMode)mode, k, S, single != 0, target);
        if (p.block == 0) {
            puts("none");
            continue;
        }
        const PlayRow &r = p.shape();
        auto tf = [](bool b) { return b ? "true" : "false"; };
        printf("%d %d %zu %d %d %d %d %d ", p.block, p.grid, p.lds, (int)p.lds_tally, (int)r.lean, (int)r.gs, (int)r.blk, (int)r.hc);
        if (r.hc) printf("fk_play_hc_kernel<%d, {m}, %s, %d, %d, %s, %s, %d>\n", r.block, tf(r.lt), r.ki, r.wpe, tf(r.pkr), tf(r.cl), r.ns);
        else printf("fk_play_kernel<%d, %s, %d, {m}, %s, %s, %d>\n", r.block, tf(r.lean), r.wpe, tf(r.gs), tf(r.blk), r.kc);
    }
    return feof(stdin) ? 0 : 1;
}
