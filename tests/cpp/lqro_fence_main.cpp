// A compiled C++ consumer of lqro::Simulator::setFence / setUserPlanes
// (include/lqro_sim.hpp), built with plain g++ against liblqro.so as
// tests/cpp/lqro_sim_main.cpp is.
// usage: lqro_fence_main IN
//   IN : int32 N, H, NP, steps; N*16 x; N*3 vGoal; 3 lo; 3 hi; tau (doubles);
//        (N + 1) int64 plane offsets; 6 floats per plane
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
  int32_t hdr[4];
  if (std::fread(hdr, sizeof hdr, 1, in) != 1) return 2;
  const int N = hdr[0], H = hdr[1], NP = hdr[2], steps = hdr[3];
  std::vector<double> x(N * 16), vg(N * 3), box(7);
  std::vector<int64_t> offs(N + 1);
  if (std::fread(x.data(), sizeof(double), x.size(), in) != x.size() ||
      std::fread(vg.data(), sizeof(double), vg.size(), in) != vg.size() ||
      std::fread(box.data(), sizeof(double), box.size(), in) != box.size() ||
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
    lqro::Simulator sim(qlist, H, NP);
    sim.findMatrices();
    sim.setFence({box[0], box[1], box[2]}, {box[3], box[4], box[5]}, box[6]);
    sim.setUserPlanes(planes);
    for (int t = 0; t < steps; ++t) {
      sim.step();
      for (int i = 0; i < N; ++i)
        std::printf("%d %d %a %a %a\n", t, i, qlist[i].newV[0], qlist[i].newV[1], qlist[i].newV[2]);
    }
  } catch (const lqro::Error& e) {
    std::fprintf(stderr, "lqro_fence_main: %s\n", e.what());
    return 1;
  }
  return 0;
}
