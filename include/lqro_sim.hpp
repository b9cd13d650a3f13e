// lqro_sim.hpp — header-only C++ host side of liblqro.so, shaped like the
// reference simulator's agent loop so that it drops into it.
//
// Reference (hihixuyang/LQR-Obstacles, QuadrotorHoverController/):
//   class Quadrotor            LQRObstacles.cpp:73-165 (the fields the loop uses)
//   findMatrices / setup       LQRObstacles.cpp:1370-1373 (controlMatrices per agent)
//   the pair loop              LQRObstacles.cpp:1391-1436  -> Simulator::step()
//   the agent loop             LQRObstacles.cpp:1437-1446  -> Simulator::update()
//   simulator2.h:34-45         the prototypes of f, h, the filters and controllers
//                              these two calls replace on the GPU
//
// Everything numeric runs in liblqro.so through the C-ABI of lqro.h; this
// header only gathers the agents' fields into the flat arrays the ABI takes
// and scatters the results back.  Matrices are row-major double arrays, the
// element order of the reference's Matrix<R,C> (include/matrix.h:16,48).
// A non-zero status from the library is thrown as lqro::Error (the C-ABI
// itself never throws).
#ifndef LQRO_SIM_HPP
#define LQRO_SIM_HPP

#include <algorithm>
#include <array>
#include <cstdint>
#include <utility>
#include <stdexcept>
#include <string>
#include <vector>

#include "lqro.h"

namespace lqro {

constexpr int kX = 16, kU = 4, kV = 3;

struct Error : std::runtime_error {
  int status;
  Error(const std::string& what, int s) : std::runtime_error(what + ": " + lqro_status_string(s)), status(s) {}
};

inline void check(int s, const char* what) {
  if (s != LQRO_OK) throw Error(what, s);
}

// The Quadrotor fields of LQRO:73-165 that the pair loop and the agent loop
// read and write.
struct Quadrotor {
  std::array<double, kX> x{};                 // estimate (State x)
  std::array<double, 9> Rot{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
  std::array<double, kX> xTrue{};
  std::array<double, 9> RotTrue{{1, 0, 0, 0, 1, 0, 0, 0, 1}};
  std::array<double, kX * kX> P{};
  std::array<double, kV> vGoal{}, newV{}, pGoal{};
  std::array<double, kU> uGoal{};
  std::array<double, kU * kX> L{};
  std::array<double, kU * kV> E{};
  std::array<double, kU> l{};
  std::array<double, kV * kX> Lh{};
  std::array<double, kV * kV> Eh{};

  // setupQuadrotors (LQRO:107-122) without its initial noise draw: xTrue = x,
  // RotTrue = Rot, P = p0 I, uGoal = hover
  void setup(const std::array<double, kX>& x0, const std::array<double, kV>& p_goal, double hover,
             double p0 = 1e-9) {
    x = x0;
    xTrue = x0;
    pGoal = p_goal;
    for (int k = 0; k < kU; ++k) uGoal[k] = hover;
    for (int k = 0; k < kX * kX; ++k) P[k] = (k % (kX + 1) == 0) ? p0 : 0.0;
  }
};

// One extra half-plane of an agent's LP (lqro_set_user_planes): a velocity v
// satisfies it when normal.(v - point) >= 0.
struct Plane { float point[3], normal[3]; };
static_assert(sizeof(Plane) == 6 * sizeof(float), "Plane is lqro_set_user_planes' six floats");

// per-agent plane lists as lqro_set_user_planes' flat arrays
inline void flatten_planes(const std::vector<std::vector<Plane>>& planes, std::vector<float>& flat,
                           std::vector<int64_t>& offsets) {
  offsets.assign(planes.size() + 1, 0);
  flat.clear();
  for (size_t i = 0; i < planes.size(); ++i) {
    for (const Plane& p : planes[i]) {
      flat.insert(flat.end(), p.point, p.point + 3);
      flat.insert(flat.end(), p.normal, p.normal + 3);
    }
    offsets[i + 1] = offsets[i] + (int64_t)planes[i].size();
  }
}

class Simulator {
 public:
  // qlist is held by reference, as the reference's qlist of Quadrotor*.
  Simulator(std::vector<Quadrotor>& qlist, int horizon, int n_points = 100, int device = 0)
      : q_(qlist), device_(device) {
    lqro_model_default(&model_);
    lqro_config cfg;
    lqro_config_default(&cfg, (int32_t)q_.size(), horizon, n_points);
    cfg.device = device;
    check(lqro_create(&cfg, &ctx_), "lqro_create");
    const size_t n = q_.size();
    xs_.resize(n * kX);
    vg_.resize(n * kV);
    nv_.resize(n * kV);
  }
  ~Simulator() { lqro_destroy(ctx_); }
  Simulator(const Simulator&) = delete;
  Simulator& operator=(const Simulator&) = delete;

  const lqro_model& model() const { return model_; }

  // controlMatrices at hover for every agent (LQRO:1370-1373): one synthesis,
  // the same L, E, Lh, Eh for all agents as in the reference; A, B feed the
  // pair loop's findFG (LQRO:1265-1266).
  void findMatrices() {
    std::vector<double> c(kX);
    check(lqro_synthesize_gains_x(&model_, kX, A_.data(), B_.data(), c.data(), q_[0].L.data(), q_[0].E.data(),
                                  q_[0].l.data(), q_[0].Lh.data(), q_[0].Eh.data()),
          "lqro_synthesize_gains_x");
    for (auto& q : q_) {
      q.L = q_[0].L; q.E = q_[0].E; q.l = q_[0].l; q.Lh = q_[0].Lh; q.Eh = q_[0].Eh;
    }
    check(lqro_set_gains(ctx_, A_.data(), B_.data(), q_[0].L.data(), q_[0].E.data(), 0), "lqro_set_gains");
  }

  // Opt-in constraints that are not agents, ahead of the pair planes in each
  // agent's LP (RVO2's obstacle-first order, AGT:84-151; no counterpart in
  // LQRO, so results change against the reference once set).  setFence: an
  // axis-aligned box the ellipsoids should stay inside within tau seconds
  // (lqro_set_fence; an infinite bound emits no face, tau <= 0 turns it off).
  // setUserPlanes: one list per agent, empty lists allowed; an empty vector
  // clears (lqro_set_user_planes).
  void setFence(const std::array<double, 3>& lo, const std::array<double, 3>& hi, double tau) {
    check(lqro_set_fence(ctx_, lo.data(), hi.data(), tau), "lqro_set_fence");
  }
  void setUserPlanes(const std::vector<std::vector<Plane>>& planes) {
    if (planes.empty()) return check(lqro_set_user_planes(ctx_, nullptr, nullptr), "lqro_set_user_planes");
    if (planes.size() != q_.size()) throw Error("setUserPlanes: one list per agent", LQRO_E_ARG);
    std::vector<float> flat;
    std::vector<int64_t> offs;
    flatten_planes(planes, flat, offs);
    flat.resize(std::max<size_t>(flat.size(), 6));   // (never a null array: NULL means clear)
    check(lqro_set_user_planes(ctx_, flat.data(), offs.data()), "lqro_set_user_planes");
  }

  // Obstacles: bodies that are not agents as extra columns of every agent's
  // pair loop (lqro_set_obstacles; the reference's commented floor block,
  // LQRO:1377-1379, 1421-1434).  One state of kX doubles each (position
  // [0..2], velocity [3..5], hover trim otherwise); radii of the obstacles'
  // ellipsoid ((0, 0): a point, LQRO:752-767); responsibility in (0, 1] for
  // the 0.5 of LQRO:1416 (1.0: the agent does all the avoiding).  An empty
  // vector clears.  Results change against the reference once set.
  void setObstacles(const std::vector<std::array<double, kX>>& states, double xy_radius, double z_radius,
                    double responsibility = 1.0) {
    std::vector<double> flat;
    for (const auto& st : states) flat.insert(flat.end(), st.begin(), st.end());
    check(lqro_set_obstacles(ctx_, flat.empty() ? nullptr : flat.data(), (int32_t)states.size(), xy_radius, z_radius,
                             responsibility),
          "lqro_set_obstacles");
  }
  // The same with a shape and a responsibility per obstacle
  // (lqro_set_obstacles_ex): three vectors of states.size() values, an empty
  // one standing for the default (the agents' radii; responsibility 1.0).
  void setObstacles(const std::vector<std::array<double, kX>>& states, const std::vector<double>& xy_radius,
                    const std::vector<double>& z_radius, const std::vector<double>& responsibility) {
    std::vector<double> flat;
    for (const auto& st : states) flat.insert(flat.end(), st.begin(), st.end());
    for (const std::vector<double>* v : {&xy_radius, &z_radius, &responsibility})
      if (!v->empty() && v->size() != states.size()) check(LQRO_E_ARG, "setObstacles: one value per obstacle");
    check(lqro_set_obstacles_ex(ctx_, flat.empty() ? nullptr : flat.data(), (int32_t)states.size(),
                                xy_radius.empty() ? nullptr : xy_radius.data(),
                                z_radius.empty() ? nullptr : z_radius.data(),
                                responsibility.empty() ? nullptr : responsibility.data()),
          "lqro_set_obstacles_ex");
  }

  // Hard planes (lqro_set_hard_planes): level LQRO_HARD_FENCE keeps the fence
  // planes out of linearProgram4's relaxation, LQRO_HARD_HEAD the user planes
  // too, LQRO_HARD_OBSTACLES also the obstacle columns' planes, which the LP
  // then takes ahead of the agent planes (RVO2's obstacle lines).  Once the
  // hard planes and the speed sphere are feasible together and the result
  // satisfies them, no later relaxation leaves them; if the hard planes are
  // infeasible among themselves nothing is guaranteed.  LQRO_HARD_NONE (the
  // default) is the reference's LP.
  void setHardPlanes(int32_t level) { check(lqro_set_hard_planes(ctx_, level), "lqro_set_hard_planes"); }

  // The activity mask (lqro_set_active): active[i] != 0, agent i takes part in
  // the steps that follow; an inactive agent is neither a row nor a column of
  // the pair loop (nobody avoids it), and step() leaves its newV at zero.  One
  // byte per agent; an empty vector clears (everybody takes part); another
  // size throws.  update() goes on propagating every agent.
  void setActive(const std::vector<uint8_t>& active) {
    if (!active.empty() && active.size() != q_.size()) throw std::runtime_error("setActive: one byte per agent");
    check(lqro_set_active(ctx_, active.empty() ? nullptr : active.data()), "lqro_set_active");
  }

  // Interaction classes (lqro_set_interaction): agent i belongs to class
  // cls[i] < n_classes, and share[a * n_classes + b] in [0, 1] is the factor a
  // row of class a applies against an agent column of class b in place of the
  // reference's 0.5; exactly 0: the row ignores the column.  One byte per
  // agent and n_classes squared shares; an empty cls clears (no table);
  // another size throws.
  void setInteraction(const std::vector<uint8_t>& cls, int32_t n_classes, const std::vector<double>& share) {
    if (cls.empty()) {
      check(lqro_set_interaction(ctx_, nullptr, 0, nullptr), "lqro_set_interaction");
      return;
    }
    if (cls.size() != q_.size()) throw std::runtime_error("setInteraction: one byte per agent");
    if (n_classes < 1 || share.size() != (size_t)n_classes * (size_t)n_classes)
      throw std::runtime_error("setInteraction: n_classes squared shares");
    check(lqro_set_interaction(ctx_, cls.data(), n_classes, share.data()), "lqro_set_interaction");
  }

  // Clearance (lqro_clearance): how clear every agent's current estimate
  // Quadrotor::x is of every other agent and obstacle, and of the fence;
  // rows, when given, receives one record per agent.  Returns the total.
  lqro_clearance_total clearance(std::vector<lqro_clearance_row>* rows = nullptr) {
    for (size_t i = 0; i < q_.size(); ++i)
      for (int c = 0; c < kX; ++c) xs_[i * kX + c] = q_[i].x[c];
    if (rows) rows->resize(q_.size());
    lqro_clearance_total t;
    check(lqro_clearance(ctx_, xs_.data(), rows ? rows->data() : nullptr, &t), "lqro_clearance");
    return t;
  }
  // The per-step monitor (lqro_set_monitor): with on, every step() measures
  // the x it reads, on the device; monitor() returns the last step's total
  // and, in *since_reset when given, the one accumulated since the last reset.
  void setMonitor(bool on) { check(lqro_set_monitor(ctx_, on ? 1 : 0), "lqro_set_monitor"); }
  lqro_clearance_total monitor(lqro_clearance_total* since_reset = nullptr, bool reset = false) {
    lqro_clearance_total last;
    check(lqro_get_monitor(ctx_, &last, since_reset, reset ? 1 : 0), "lqro_get_monitor");
    return last;
  }

  // Horizon conflict prediction (lqro_predict): with every agent's current
  // estimate Quadrotor::x and the velocity newV the last step() chose, does
  // the closed loop keep each pair apart over the horizon, and if not, when
  // and with whom does it first fail?  rows, when given, receives one record
  // per agent.  Returns this prediction's total.  (lqro::ShardedSimulator has
  // no counterpart: a rank predicts with its own context, the caller merges.)
  lqro_predict_total predict(std::vector<lqro_predict_row>* rows = nullptr) {
    std::vector<double> v(q_.size() * kV);
    for (size_t i = 0; i < q_.size(); ++i) {
      for (int c = 0; c < kX; ++c) xs_[i * kX + c] = q_[i].x[c];
      for (int c = 0; c < kV; ++c) v[i * kV + c] = q_[i].newV[c];
    }
    if (rows) rows->resize(q_.size());
    lqro_predict_total t;
    check(lqro_predict(ctx_, xs_.data(), v.data(), rows ? rows->data() : nullptr, &t), "lqro_predict");
    return t;
  }

  // The LP audit (lqro_set_lp_audit): with on, every step() measures its
  // result against each plane the agent's LP saw, on the device; tol >= 0 is
  // the margin above which a plane counts as violated.  lp_audit() returns
  // the last step's total and, in *since_reset when given, the one
  // accumulated since the last reset; rows, when given, receives one record
  // per agent.  (lqro::ShardedSimulator has no counterpart and does not
  // merge: a rank reads its own context, the caller merges.)
  void set_lp_audit(bool on, float tol = 0.0f) { check(lqro_set_lp_audit(ctx_, on ? 1 : 0, tol), "lqro_set_lp_audit"); }
  lqro_lp_total lp_audit(lqro_lp_total* since_reset = nullptr, bool reset = false,
                        std::vector<lqro_lp_row>* rows = nullptr) {
    lqro_lp_total last;
    if (rows) {
      rows->resize(q_.size());
      int64_t n = 0;
      check(lqro_get_lp_audit_rows(ctx_, rows->data(), (int64_t)rows->size(), &n), "lqro_get_lp_audit_rows");
      rows->resize((size_t)n);
    }
    check(lqro_get_lp_audit(ctx_, &last, since_reset, reset ? 1 : 0), "lqro_get_lp_audit");
    return last;
  }

  // The pair loop LQRO:1393-1436 on the GPU: every Quadrotor::newV.
  // LQRO_E_HULL (a pair without its half-plane) and LQRO_E_QHMERGE (a pair
  // whose winning facet qconvex's pre-merge may join: its half-plane is not
  // pinned to the reference) still write newV: it is stored, then thrown
  // as lqro::Error (status(), hull_failures(), qhmerge_pairs() say which).
  void step() {
    for (size_t i = 0; i < q_.size(); ++i)
      for (int c = 0; c < kX; ++c) xs_[i * kX + c] = q_[i].x[c];
    for (size_t i = 0; i < q_.size(); ++i)
      for (int c = 0; c < kV; ++c) vg_[i * kV + c] = q_[i].vGoal[c];
    const int s = lqro_step(ctx_, xs_.data(), vg_.data(), nv_.data());
    if (s == LQRO_OK || s == LQRO_E_HULL || s == LQRO_E_QHMERGE)
      for (size_t i = 0; i < q_.size(); ++i)
        for (int c = 0; c < kV; ++c) q_[i].newV[c] = nv_[i * kV + c];
    check(s, "lqro_step");
  }

  // (i, j) of the last step's pairs lqro_get_hull_failures /
  // lqro_get_qhmerge_pairs name (at most 64 each)
  std::vector<std::pair<int, int>> hull_failures() const { return named(lqro_get_hull_failures); }
  std::vector<std::pair<int, int>> qhmerge_pairs() const { return named(lqro_get_qhmerge_pairs); }

  // The agent loop LQRO:1437-1446 on the GPU: vGoal = newV, findU,
  // propagate, kalmanFilter1, the observation draw, kalmanFilter2,
  // vGoal = findVGoal.  Noise from the reference's rand() stream at `seed`
  // (srand); returns the next seed.
  uint32_t update(uint32_t seed) {
    const size_t n = q_.size();
    std::vector<double> x(n * kX), rot(n * 9), xt(n * kX), rott(n * 9), P(n * kX * kX), vg(n * kV), ug(n * kU),
        pg(n * kV), L(n * kU * kX), E(n * kU * kV), l(n * kU), Lh(n * kV * kX), Eh(n * kV * kV),
        nrm(n * LQRO_NORMALS_PER_AGENT), M(kX * kX, 0.0), Nz(36, 0.0);
    for (int k = 0; k < kX; ++k) M[k * (kX + 1)] = 1e-9;   // LQRO:1285
    for (int k = 0; k < 6; ++k) Nz[k * 7] = 1e-9;          // LQRO:1286
    auto put = [](std::vector<double>& dst, size_t i, const double* src, size_t len) {
      for (size_t k = 0; k < len; ++k) dst[i * len + k] = src[k];
    };
    for (size_t i = 0; i < n; ++i) {
      const Quadrotor& q = q_[i];
      put(x, i, q.x.data(), kX); put(rot, i, q.Rot.data(), 9); put(xt, i, q.xTrue.data(), kX);
      put(rott, i, q.RotTrue.data(), 9); put(P, i, q.P.data(), kX * kX);
      put(vg, i, q.newV.data(), kV);   // vGoal = newV (LQRO:1438)
      put(ug, i, q.uGoal.data(), kU); put(pg, i, q.pGoal.data(), kV);
      put(L, i, q.L.data(), kU * kX); put(E, i, q.E.data(), kU * kV); put(l, i, q.l.data(), kU);
      put(Lh, i, q.Lh.data(), kV * kX); put(Eh, i, q.Eh.data(), kV * kV);
    }
    check(lqro_normals(&seed, (int64_t)nrm.size(), nrm.data()), "lqro_normals");
    lqro_agents a;
    a.x = x.data(); a.rot = rot.data(); a.x_true = xt.data(); a.rot_true = rott.data(); a.P = P.data();
    a.vgoal = vg.data(); a.u = nullptr; a.u_goal = ug.data(); a.p_goal = pg.data();
    a.L = L.data(); a.E = E.data(); a.l = l.data(); a.Lh = Lh.data(); a.Eh = Eh.data();
    a.M = M.data(); a.N = Nz.data(); a.normals = nrm.data(); a.keyframes = nullptr;
    a.time = t_ * model_.dt;
    check(lqro_dynamics_step(&model_, 1, (int32_t)n, 1, &a, device_), "lqro_dynamics_step");
    auto get = [](std::vector<double>& src, size_t i, double* dst, size_t len) {
      for (size_t k = 0; k < len; ++k) dst[k] = src[i * len + k];
    };
    for (size_t i = 0; i < n; ++i) {
      Quadrotor& q = q_[i];
      get(x, i, q.x.data(), kX); get(rot, i, q.Rot.data(), 9); get(xt, i, q.xTrue.data(), kX);
      get(rott, i, q.RotTrue.data(), 9); get(P, i, q.P.data(), kX * kX); get(vg, i, q.vGoal.data(), kV);
    }
    ++t_;
    return seed;
  }

 private:
  std::vector<std::pair<int, int>> named(int (*get)(lqro_ctx*, int64_t*, int64_t, int64_t*)) const {
    int64_t p[128], n = 0;
    check(get(ctx_, p, 64, &n), "lqro_get_*_pairs");
    std::vector<std::pair<int, int>> out;
    for (int64_t k = 0; k < std::min<int64_t>(n, 64); ++k) out.emplace_back((int)p[2 * k], (int)p[2 * k + 1]);
    return out;
  }

  std::vector<Quadrotor>& q_;
  int device_;
  lqro_model model_;
  lqro_ctx* ctx_ = nullptr;
  std::array<double, kX * kX> A_{};
  std::array<double, kX * kU> B_{};
  std::vector<double> xs_, vg_, nv_;
  int t_ = 0;
};

}  // namespace lqro
#endif  // LQRO_SIM_HPP
