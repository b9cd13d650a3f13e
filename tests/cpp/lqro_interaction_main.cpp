// lqro::Simulator's setInteraction, compiled with plain g++ against liblqro.so
// as tests/cpp/lqro_sim_main.cpp is.
// usage: lqro_interaction_main IN OUT
//   IN : int32 N, H, NP, steps, C; N*16 x; N*3 vGoal (doubles); C*C shares
//        (doubles); steps x N class bytes (a step whose bytes are all 255
//        clears the table instead)
//   OUT: per step: N*3 newV (doubles), the pair loop alone: x and vGoal stay
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
  const int N = hdr[0], H = hdr[1], NP = hdr[2], steps = hdr[3], C = hdr[4];
  if (C < 1 || C > LQRO_CLASSES_MAX) return 2;
  std::vector<double> x(N * 16), vg(N * 3), share((size_t)C * C);
  for (std::vector<double>* v : {&x, &vg, &share})
    if (std::fread(v->data(), sizeof(double), v->size(), in) != v->size()) return 2;
  std::vector<uint8_t> classes((size_t)steps * N);
  if (std::fread(classes.data(), 1, classes.size(), in) != classes.size()) return 2;
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
    for (int t = 0; t < steps; ++t) {
      std::vector<uint8_t> k(classes.begin() + (size_t)t * N, classes.begin() + (size_t)(t + 1) * N);
      bool clear = true;
      for (uint8_t b : k) clear = clear && b == 255;
      sim.setInteraction(clear ? std::vector<uint8_t>() : k, C, share);
      try {
        sim.step();
      } catch (const lqro::Error& e) {   // (a merge suspect or a failed hull still completes the step)
        if (e.status != LQRO_E_HULL && e.status != LQRO_E_QHMERGE) throw;
      }
      for (const auto& q : qlist) std::fwrite(q.newV.data(), sizeof(double), 3, out);
      std::printf("step %d: %s\n", t, clear ? "no table" : "table set");
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "lqro_interaction_main: %s\n", e.what());
    std::fclose(out);
    return 1;
  }
  std::fclose(out);
  return 0;
}
