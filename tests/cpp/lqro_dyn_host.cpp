// lqro_dyn_host.cpp — the host side of lqro_dyn.hpp's dyn::agent_step (the
// text k_dyn compiles for the device) behind one C function, for ctypes
// (tests/test_dyn_hard_cpu.py): with the library's floating-point flags it
// must give the oracle's orc_agent_step bit for bit, so a difference on the
// GPU is the device's arithmetic and not the restatement.
#include "../../lqr-obstacles_amd/csrc/lqro_dyn.hpp"

// One agent.  keyframe8 and u_out may be null.
extern "C" void lqro_dyn_host_agent_step(const lqro_model* model, const double* L, const double* E,
                                         const double* l, const double* Lh, const double* Eh,
                                         const double* u_goal, const double* p_goal, const double* M,
                                         const double* Nz, const double* normals, double time,
                                         double* x, double* rot, double* x_true, double* rot_true,
                                         double* P, double* vgoal, double* u_out, float* keyframe8) {
  lqro::dyn::AgentParams a;
  a.model = model;
  a.L = L; a.E = E; a.l = l; a.Lh = Lh; a.Eh = Eh;
  a.u_goal = u_goal; a.p_goal = p_goal;
  a.M = M; a.Nz = Nz;
  a.normals = normals;
  a.keyframe = keyframe8;
  a.time = time;
  lqro::dyn::agent_step(a, x, rot, x_true, rot_true, P, vgoal, u_out);
}
