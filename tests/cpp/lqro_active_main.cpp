// lqro::Simulator's setActive, compiled with plain g++ against liblqro.so as
// tests/cpp/lqro_sim_main.cpp is.
// usage: lqro_active_main IN OUT
//   IN : int32 N, H, NP, steps; N*16 x; N*3 vGoal (doubles); steps x N mask
//        bytes (a step whose bytes are all 255 clears the mask instead)
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
  int32_t hdr[4];
  if (std::fread(hdr, sizeof hdr, 1, in) != 1) return 2;
  const int N = hdr[0], H = hdr[1], NP = hdr[2], steps = hdr[3];
  std::vector<double> x(N * 16), vg(N * 3);
  for (std::vector<double>* v : {&x, &vg})
    if (std::fread(v->data(), sizeof(double), v->size(), in) != v->size()) return 2;
  std::vector<uint8_t> masks((size_t)steps * N);
  if (std::fread(masks.data(), 1, masks.size(), in) != masks.size()) return 2;
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
      std::vector<uint8_t> a(masks.begin() + (size_t)t * N, masks.begin() + (size_t)(t + 1) * N);
      bool clear = true;
      for (uint8_t b : a) clear = clear && b == 255;
      sim.setActive(clear ? std::vector<uint8_t>() : a);
      try {
        sim.step();
      } catch (const lqro::Error& e) {   // (a merge suspect or a failed hull still completes the step)
        if (e.status != LQRO_E_HULL && e.status != LQRO_E_QHMERGE) throw;
      }
      int on = 0;
      for (uint8_t b : a) on += b != 0;
      for (const auto& q : qlist) std::fwrite(q.newV.data(), sizeof(double), 3, out);
      std::printf("step %d: %d of %d agents active\n", t, on, N);
    }
  } catch (const std::exception& e) {
    std::fprintf(stderr, "lqro_active_main: %s\n", e.what());
    std::fclose(out);
    return 1;
  }
  std::fclose(out);
  return 0;
}
