// k_pair's LDS layout (lqro_plan.hpp pair_layout) for "H:NP:X:K" arguments,
// K = obstacle shape classes that are not the agents' (lqro_set_obstacles_ex).
// One line per argument.  Host only: built with g++, also under
// -fsanitize=address,undefined (tests/test_obstacle_shapes_cpu.py).
#include <cstdio>

#include "lqro_plan.hpp"

int main(int argc, char** argv) {
  for (int a = 1; a < argc; ++a) {
    int H = 0, NP = 0, X = 0, K = 0;
    if (std::sscanf(argv[a], "%d:%d:%d:%d", &H, &NP, &X, &K) != 4) {
      std::fprintf(stderr, "usage: %s H:NP:X:K ...\n", argv[0]);
      return 2;
    }
    lqro::PairLayout L{};
    const bool ok = lqro::pair_layout(H, NP, X, K, L);
    std::printf("H=%d NP=%d X=%d K=%d ok=%d T=%d N=%d S=%d R=%d TF=%d Hh=%d cls=%d cls_doubles=%d wave=%d "
                "wave_doubles=%d waves=%d bytes=%d\n",
                H, NP, X, K, ok ? 1 : 0, L.lds_T, L.lds_N, L.lds_S, L.lds_R, L.lds_TF, L.lds_H, L.lds_cls,
                L.cls_doubles, L.lds_wave, L.wave_doubles, L.waves, L.lds_bytes);
  }
  return 0;
}
