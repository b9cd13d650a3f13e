// A compiled C++ consumer of lqro::Simulator::setHardPlanes
// (include/lqro_sim.hpp) over a fence, user planes and obstacles, built with
// plain g++ against liblqro.so as tests/cpp/lqro_sim_main.cpp is.
// usage: lqro_hard_main IN
//   IN : int32 N, H, NP, steps, M, level; N*16 x; N*3 vGoal; 3 lo; 3 hi; tau
//        (doubles); M*16 obstacle states; obstacle xy radius, z radius,
//        responsibility (doubles); (N + 1) int64 plane offsets; 6 floats per
//        plane
//   stdout: per step and agent one line "t i newV.x newV.y newV.z" as
//        hexadecimal floats (every step from the same x and vGoal)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lqro_sim.hpp"

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s IN\n", argv[0]);
    return 2;
  }
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t hdr[6];
  if (std::fread(hdr, sizeof hdr, 1, in) != 1) return 2;
  const int N = hdr[0], H = hdr[1], NP = hdr[2], steps = hdr[3], M = hdr[4], level = hdr[5];
  std::vector<double> x(N * 16), vg(N * 3), box(7), ob((size_t)M * 16), par(3);
  std::vector<int64_t> offs(N + 1);
  if (std::fread(x.data(), sizeof(double), x.size(), in) != x.size() ||
      std::fread(vg.data(), sizeof(double), vg.size(), in) != vg.size() ||
      std::fread(box.data(), sizeof(double), box.size(), in) != box.size() ||
      (M > 0 && std::fread(ob.data(), sizeof(double), ob.size(), in) != ob.size()) ||
      std::fread(par.data(), sizeof(double), par.size(), in) != par.size() ||
      std::fread(offs.data(), sizeof(int64_t), offs.size(), in) != offs.size())
    return 2;
  std::vector<std::vector<lqro::Plane>> planes(N);
  for (int i = 0; i < N; ++i) {
    planes[i].resize((size_t)(offs[i + 1] - offs[i]));
    if (!planes[i].empty() &&
        std::fread(planes[i].data(), sizeof(lqro::Plane), planes[i].size(), in) != planes[i].size())
      return 2;
  }
  std::fclose(in);
  try {
    std::vector<lqro::Quadrotor> qlist(N);
    for (int i = 0; i < N; ++i) {
      for (int c = 0; c < 16; ++c) qlist[i].x[c] = x[i * 16 + c];
      for (int c = 0; c < 3; ++c) qlist[i].vGoal[c] = vg[i * 3 + c];
    }
    std::vector<std::array<double, lqro::kX>> obs(M);
    for (int o = 0; o < M; ++o)
      for (int c = 0; c < 16; ++c) obs[o][c] = ob[o * 16 + c];
    lqro::Simulator sim(qlist, H, NP);
    sim.findMatrices();
    sim.setHardPlanes(level);   // (first: the level stays through the calls below)
    sim.setFence({box[0], box[1], box[2]}, {box[3], box[4], box[5]}, box[6]);
    sim.setUserPlanes(planes);
    sim.setObstacles(obs, par[0], par[1], par[2]);
    for (int t = 0; t < steps; ++t) {
      sim.step();
      for (int i = 0; i < N; ++i)
        std::printf("%d %d %a %a %a\n", t, i, qlist[i].newV[0], qlist[i].newV[1], qlist[i].newV[2]);
    }
  } catch (const lqro::Error& e) {
    std::fprintf(stderr, "lqro_hard_main: %s\n", e.what());
    return 1;
  }
  return 0;
}
