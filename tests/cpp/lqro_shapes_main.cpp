// lqro::Simulator::setObstacles and lqro::ShardedSimulator::setObstacles with
// a shape and a responsibility per obstacle (the std::vector overloads over
// lqro_set_obstacles_ex): both hosts run the reference's agent loop
// (LQRObstacles.cpp:1391-1446) from the same swarm and rand() seed; the
// sharded host as a world of one rank, as tests/cpp/lqro_sharded_main.cpp does.
// usage: lqro_shapes_main IN OUT
//   IN : int32 N, H, NP, steps, M; uint32 seed; N*16 x; N*3 vGoal; N*3 pGoal;
//        M*16 obstacle states; M xy radii; M z radii; M responsibilities
//   OUT: per step: Simulator newV (N*3), x (N*16); ShardedSimulator newV (N*3), x (N*16)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "lqro_sharded.hpp"

static std::vector<lqro::Quadrotor> swarm(int N, const std::vector<double>& x, const std::vector<double>& vg,
                                          const std::vector<double>& pg) {
  std::vector<lqro::Quadrotor> qlist(N);
  lqro_model m;
  lqro_model_default(&m);
  const double hover = m.gravity * m.mass / 4;   // nominalInput (LQRO:188)
  for (int i = 0; i < N; ++i) {
    std::array<double, 16> xi;
    std::array<double, 3> pgi;
    for (int c = 0; c < 16; ++c) xi[c] = x[i * 16 + c];
    for (int c = 0; c < 3; ++c) pgi[c] = pg[i * 3 + c];
    qlist[i].setup(xi, pgi, hover);
    for (int c = 0; c < 3; ++c) qlist[i].vGoal[c] = vg[i * 3 + c];
  }
  return qlist;
}

int main(int argc, char** argv) {
  if (argc != 3) {
    std::fprintf(stderr, "usage: %s IN OUT\n", argv[0]);
    return 2;
  }
  FILE* in = std::fopen(argv[1], "rb");
  if (!in) return 2;
  int32_t hdr[5];
  uint32_t seed = 0;
  if (std::fread(hdr, sizeof hdr, 1, in) != 1 || std::fread(&seed, sizeof seed, 1, in) != 1) return 2;
  const int N = hdr[0], H = hdr[1], NP = hdr[2], steps = hdr[3], M = hdr[4];
  if (N < 1 || M < 1) return 2;
  std::vector<double> x(N * 16), vg(N * 3), pg(N * 3), ob((size_t)M * 16), oxy(M), oz(M), resp(M);
  for (std::vector<double>* v : {&x, &vg, &pg, &ob, &oxy, &oz, &resp})
    if (std::fread(v->data(), sizeof(double), v->size(), in) != v->size()) return 2;
  std::fclose(in);
  FILE* out = std::fopen(argv[2], "wb");
  if (!out) return 2;
  try {
    std::vector<lqro::Quadrotor> qa = swarm(N, x, vg, pg), qb = swarm(N, x, vg, pg);
    std::vector<std::array<double, lqro::kX>> obs(M);
    for (int o = 0; o < M; ++o)
      for (int c = 0; c < 16; ++c) obs[o][c] = ob[o * 16 + c];
    // the one-GPU host first: without a gfx950 device this throws before RCCL is touched
    lqro::Simulator sim(qa, H, NP);
    sim.findMatrices();
    sim.setObstacles(obs, oxy, oz, resp);
    ncclUniqueId id;
    lqro::check_nccl(ncclGetUniqueId(&id), "ncclGetUniqueId");
    lqro::ShardedSimulator sh(qb, H, NP, 0, 1, id);
    sh.findMatrices();
    sh.setObstacles(obs, oxy, oz, resp);
    uint32_t sa = seed, sb = seed;
    for (int t = 0; t < steps; ++t) {
      sim.step();
      sa = sim.update(sa);
      sb = sh.iterate(sb);
      sh.download();
      for (const auto& q : qa) std::fwrite(q.newV.data(), sizeof(double), 3, out);
      for (const auto& q : qa) std::fwrite(q.x.data(), sizeof(double), 16, out);
      for (const auto& q : qb) std::fwrite(q.newV.data(), sizeof(double), 3, out);
      for (const auto& q : qb) std::fwrite(q.x.data(), sizeof(double), 16, out);
    }
  } catch (const lqro::Error& e) {
    std::fprintf(stderr, "lqro_shapes_main: %s\n", e.what());
    std::fclose(out);
    return 1;
  }
  std::fclose(out);
  return 0;
}
