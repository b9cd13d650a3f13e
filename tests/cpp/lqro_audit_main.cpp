// lqro::Simulator's set_lp_audit and lp_audit, compiled with plain g++ against
// liblqro.so as tests/cpp/lqro_sim_main.cpp is.
// usage: lqro_audit_main IN OUT
//   IN : int32 N, H, NP, steps, fence, hard; float tol; N*16 x; N*3 vGoal;
//        lo[3]; hi[3]; tau (doubles; the box is set when fence != 0)
//   OUT: per step: N*3 newV, lp_audit()'s last total, its since-reset total,
//        its N lqro_lp_row
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
  int32_t hdr[6];
  float tol = 0.0f;
  if (std::fread(hdr, sizeof hdr, 1, in) != 1 || std::fread(&tol, sizeof tol, 1, in) != 1) return 2;
  const int N = hdr[0], H = hdr[1], NP = hdr[2], steps = hdr[3], fence = hdr[4], hard = hdr[5];
  std::vector<double> x(N * 16), vg(N * 3), box(7);
  for (std::vector<double>* v : {&x, &vg, &box})
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
    if (fence) sim.setFence({box[0], box[1], box[2]}, {box[3], box[4], box[5]}, box[6]);
    sim.setHardPlanes(hard);
    sim.set_lp_audit(true, tol);
    sim.findMatrices();
    for (int t = 0; t < steps; ++t) {
      try {
        sim.step();
      } catch (const lqro::Error& e) {   // (a merge suspect or a failed hull still completes the step)
        if (e.status != LQRO_E_HULL && e.status != LQRO_E_QHMERGE) throw;
      }
      std::vector<lqro_lp_row> rows;
      lqro_lp_total since;
      const lqro_lp_total last = sim.lp_audit(&since, false, &rows);
      for (const auto& q : qlist) std::fwrite(q.newV.data(), sizeof(double), 3, out);
      std::fwrite(&last, sizeof last, 1, out);
      std::fwrite(&since, sizeof since, 1, out);
      std::fwrite(rows.data(), sizeof(lqro_lp_row), rows.size(), out);
      std::printf("step %d: viol_max %.9g (row %d, plane %d, kind %d, id %d), %lld rows over tol, %lld planes\n", t,
                  last.viol_max, last.viol_i, last.viol_k, last.viol_kind, last.viol_id,
                  (long long)last.n_rows_viol, (long long)last.n_planes);
    }
  } catch (const lqro::Error& e) {
    std::fprintf(stderr, "lqro_audit_main: %s\n", e.what());
    std::fclose(out);
    return 1;
  }
  std::fclose(out);
  return 0;
}
