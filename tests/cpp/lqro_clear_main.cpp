// lqro::Simulator's clearance, setMonitor and monitor, compiled with plain
// g++ against liblqro.so as tests/cpp/lqro_sim_main.cpp is.
// usage: lqro_clear_main IN OUT
//   IN : int32 N, H, NP, M, fence; N*16 x; M*16 obstacle states; M xy radii;
//        M z radii; lo[3]; hi[3] (doubles; the box is set when fence != 0)
//   OUT: lqro_clearance_total of clearance(); its N lqro_clearance_row; then,
//        after setMonitor(true) and one step(), monitor()'s last total and
//        its since-reset total
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lqro_sim.hpp"

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t hdr[5];
  if (std::fread(hdr, sizeof hdr, 1, in) != 1) return 2;
  const int N = hdr[0], H = hdr[1], NP = hdr[2], M = hdr[3], fence = hdr[4];
  std::vector<double> x(N * 16), obs(M * 16), oxy(M), oz(M), box(6);
  for (std::vector<double>* v : {&x, &obs, &oxy, &oz, &box})
    if (!v->empty() && std::fread(v->data(), sizeof(double), v->size(), in) != v->size()) return 2;
  std::fclose(in);
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  try {
    std::vector<lqro::Quadrotor> qlist(N);
    lqro_model m;
    lqro_model_default(&m);
    const double hover = m.gravity * m.mass / 4;
    for (int i = 0; i < N; ++i) {
      std::array<double, 16> xi;
      for (int c = 0; c < 16; ++c) xi[c] = x[i * 16 + c];
      qlist[i].setup(xi, {0.0, 0.0, 0.0}, hover);
    }
    lqro::Simulator sim(qlist, H, NP);
    if (M > 0) {
      std::vector<std::array<double, 16>> st(M);
      for (int o = 0; o < M; ++o)
        for (int c = 0; c < 16; ++c) st[o][c] = obs[o * 16 + c];
      sim.setObstacles(st, oxy, oz, {});
    }
    if (fence) sim.setFence({box[0], box[1], box[2]}, {box[3], box[4], box[5]}, 1.0);
    std::vector<lqro_clearance_row> rows;
    const lqro_clearance_total t = sim.clearance(&rows);
    std::fwrite(&t, sizeof t, 1, out);
    std::fwrite(rows.data(), sizeof(lqro_clearance_row), rows.size(), out);
    sim.setMonitor(true);
    sim.findMatrices();
    try {
      sim.step();
    } catch (const lqro::Error& e) {   // (a merge suspect or a failed hull still completes the step)
      if (e.status != LQRO_E_HULL && e.status != LQRO_E_QHMERGE) throw;
    }
    lqro_clearance_total since;
    const lqro_clearance_total last = sim.monitor(&since);
    std::fwrite(&last, sizeof last, 1, out);
    std::fwrite(&since, sizeof since, 1, out);
    std::printf("s2_min %.17g (%d, %d) n_hit %lld n_measured %lld\n", last.s2_min, last.s2_i, last.s2_j,
                (long long)last.n_hit, (long long)since.n_measured);
  } catch (const lqro::Error& e) {
    std::fprintf(stderr, "lqro_clear_main: %s\n", e.what());
    std::fclose(out);
    return 1;
  }
  std::fclose(out);
  return 0;
}
