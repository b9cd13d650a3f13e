// lqro_plan_hard_main — plan_step (csrc/lqro_plan.hpp) on a Qhull-order
// context of 1024 rows (the steady step's feedback of the
// `c3_steady_qhull_default` case of tests/golden/step_plan.json) whose LP
// takes its obstacle slots ahead of its agent slots (lqro_set_hard_planes at
// LQRO_HARD_OBSTACLES with obstacles set: StepShape::hard_obs), for
// tests/test_hard_planes_cpu.py.
// usage: lqro_plan_hard_main NPR:M:EXTRA:LEVEL ...
// The runtime's rule for hard_obs is restated here: level 3 and M > 0.
// Prints per argument the early LP's two decisions.
#include <cstdio>
#include <cstdlib>

#include "lqro_plan.hpp"

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    int npr = 0, m = 0, extra = 0, level = 0;
    if (std::sscanf(argv[a], "%d:%d:%d:%d", &npr, &m, &extra, &level) != 4) return 2;
    lqro::StepShape s{};
    s.n_cu = 256; s.nrows = 1024; s.npr = npr; s.nbr_k = 0; s.hnp = 10000;
    s.per_agent = 0; s.qhull_order = 1; s.phase = 0; s.has_newv = true; s.newv_is_callers = true;
    s.waves = 16; s.lds_wave = 6600; s.wave_doubles = 773;
    s.hull_lds_max_hnp = 21845; s.hull_lds_doubles = 16544; s.hull_cwaves = 8; s.qhull_lds_doubles = 20436;
    s.lp_lds_max = 163840; s.early_lp_max_npr = 1024; s.row_big = 1048576;
    s.extra_planes = extra;
    s.n_obs = m;
    s.hard_obs = level >= 3 && m > 0 ? 1 : 0;
    lqro::StepKnobs k{};
    k.hot_on = 1; k.hot_split = 1; k.hot_spec = 1; k.hot_max_inside = -1; k.qside = 0; k.qside_pct = 100;
    k.qspare = 4; k.qbalance = 1; k.qhull_inline = 1; k.qhull_big = 0; k.hull_big_only = 0; k.local_hull = 1;
    k.side_cus = 96; k.lside_cus = 48; k.early_lp = 1;
    lqro::StepFeedback f = lqro::kNoFeedback;
    f.inside = 177; f.sweep_work = 132750000; f.build_work = 171690000; f.build_max = 1890000; f.retried = 0;
    const lqro::StepPlan p = lqro::plan_step(s, k, f, true);
    std::printf("npr=%d m=%d extra=%d level=%d early=%d row_lp=%d\n", npr, m, extra, level, p.early ? 1 : 0, p.row_lp);
  }
  return 0;
}
