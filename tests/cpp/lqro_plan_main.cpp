// lqro_plan_main — plan_step (csrc/lqro_plan.hpp) on cases read from stdin,
// for tests/test_step_plan.py.  One case is 41 whitespace-separated numbers:
// the StepShape fields, the StepKnobs fields the plan reads, then `known` and
// the five StepFeedback words (the order of `input_fields` in
// tests/golden/step_plan.json).  One line of name=value per case: every
// StepPlan field.
#include <cstdio>

#include "../../lqr-obstacles_amd/csrc/lqro_plan.hpp"

int main() {
  for (;;) {
    lqro::StepShape s{};
    lqro::StepKnobs k{};
    lqro::StepFeedback f = lqro::kNoFeedback;
    int has_newv, callers, known;
    if (scanf("%d %d %d %d %zu %d %d %d %d %d %d %d %d %zu %zu %d %zu %zu %d %d", &s.n_cu, &s.nrows, &s.npr, &s.nbr_k,
              &s.hnp, &s.per_agent, &s.qhull_order, &s.phase, &has_newv, &callers, &s.waves, &s.lds_wave,
              &s.wave_doubles, &s.hull_lds_max_hnp, &s.hull_lds_doubles, &s.hull_cwaves, &s.qhull_lds_doubles,
              &s.lp_lds_max, &s.early_lp_max_npr, &s.row_big) != 20)
      break;
    s.has_newv = has_newv != 0;
    s.newv_is_callers = callers != 0;
    if (scanf("%d %d %d %ld %d %d %d %d %d %d %d %d %d %d %d", &k.hot_on, &k.hot_split, &k.hot_spec, &k.hot_max_inside,
              &k.qside, &k.qside_pct, &k.qspare, &k.qbalance, &k.qhull_inline, &k.qhull_big, &k.hull_big_only,
              &k.local_hull, &k.side_cus, &k.lside_cus, &k.early_lp) != 15)
      return 2;
    unsigned long long w[5];
    if (scanf("%d %llu %llu %llu %llu %llu", &known, &w[0], &w[1], &w[2], &w[3], &w[4]) != 6) return 2;
    if (known) {
      f.inside = w[0]; f.sweep_work = w[1]; f.build_work = w[2]; f.build_max = w[3]; f.retried = w[4];
    }
    const lqro::StepPlan p = lqro::plan_step(s, k, f, known != 0);
    printf("npr=%d slots=%ld lds_ok=%d side_waves=%d qside_waves=%d hot=%d side=%d nwait=%d split=%d spec=%d qside=%d "
           "early=%d early_internal=%d row_split=%d nblk=%u nside=%u big_inline=%d row_lp=%d row_target=%d\n",
           p.npr, p.slots, (int)p.lds_ok, p.side_waves, p.qside_waves, (int)p.hot, p.side, p.nwait, (int)p.split,
           (int)p.spec, (int)p.qside, (int)p.early, (int)p.early_internal, p.row_split, p.nblk, p.nside, p.big_inline,
           p.row_lp, p.row_target);
  }
  return 0;
}
