// lqro::Simulator's predict, compiled with plain g++ against liblqro.so as
// tests/cpp/lqro_sim_main.cpp is.
// usage: lqro_predict_main IN OUT
//   IN : int32 N, H, NP; N*16 x; N*3 vGoal (doubles)
//   OUT: after findMatrices() and one step(): N*3 newV; predict()'s
//        lqro_predict_total; its N lqro_predict_row
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
  int32_t hdr[3];
  if (std::fread(hdr, sizeof hdr, 1, in) != 1) return 2;
  const int N = hdr[0], H = hdr[1], NP = hdr[2];
  std::vector<double> x(N * 16), vg(N * 3);
  for (std::vector<double>* v : {&x, &vg})
    if (std::fread(v->data(), sizeof(double), v->size(), in) != v->size()) return 2;
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
      for (int c = 0; c < 3; ++c) qlist[i].vGoal[c] = vg[i * 3 + c];
    }
    lqro::Simulator sim(qlist, H, NP);
    sim.findMatrices();
    try {
      sim.step();
    } catch (const lqro::Error& e) {   // (a merge suspect or a failed hull still completes the step)
      if (e.status != LQRO_E_HULL && e.status != LQRO_E_QHMERGE) throw;
    }
    for (const auto& q : qlist) std::fwrite(q.newV.data(), sizeof(double), 3, out);
    std::vector<lqro_predict_row> rows;
    const lqro_predict_total t = sim.predict(&rows);
    std::fwrite(&t, sizeof t, 1, out);
    std::fwrite(rows.data(), sizeof(lqro_predict_row), rows.size(), out);
    std::printf("s2_min %.17g (%d, %d, %d) first (%d, %d, %d) n_conf %lld\n", t.s2_min, t.s2_i, t.s2_j, t.s2_k,
                t.first_k, t.first_i, t.first_j, (long long)t.n_conf);
  } catch (const lqro::Error& e) {
    std::fprintf(stderr, "lqro_predict_main: %s\n", e.what());
    std::fclose(out);
    return 1;
  }
  std::fclose(out);
  return 0;
}
