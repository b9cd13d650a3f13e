/*
 * lqro.h — C-ABI of the MI355X-native LQR-Obstacle step (liblqro.so).
 *
 * This is the drop-in boundary for the per-timestep pair loop of the
 * reference simulator (hihixuyang/LQR-Obstacles,
 * QuadrotorHoverController/LQRObstacles.cpp, "LQRO" below).  The reference
 * has no plugin/FFI API: the path is a set of free functions driven by the
 * loop at LQRO:1391-1436.  Each entry point below names the reference code it
 * replaces.  Conventions:
 *   - every function returns an int status: 0 = LQRO_OK, negative = error;
 *     no C++ exception crosses the ABI;
 *   - the caller owns every host array; the context owns device buffers and
 *     its HIP stream;
 *   - one context per host thread; contexts are independent of each other;
 *   - matrices are row-major fp64, exactly the element order of the
 *     reference's Matrix<R,C> (include/matrix.h:16,48).
 */
#ifndef LQRO_H
#define LQRO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes ------------------------------------------------------ */
enum {
  LQRO_OK = 0,
  LQRO_E_ARG = -1,       /* bad argument / config                          */
  LQRO_E_HIP = -2,       /* a HIP runtime call failed                      */
  LQRO_E_NOMEM = -3,     /* device or host allocation failed               */
  LQRO_E_STATE = -4,     /* call order violated (e.g. step before gains)   */
  LQRO_E_SINGULAR = -5,  /* singular 3x3 C*G_k (reference asserts, MAT:632) */
  LQRO_E_NODEVICE = -6,  /* no usable gfx950 device                        */
  LQRO_E_OVERFLOW = -7,  /* an internal work queue overflowed              */
  LQRO_E_HULL = -8,      /* an inside-hull pair's hull could not be built    */
                         /*   (degenerate / too few points, or every hull    */
                         /*   kernel's capacity exceeded): its half-plane is */
                         /*   missing (lqro_get_hull_failures names pairs)   */
  LQRO_E_QHMERGE = -9    /* the step completed (newv written), but an inside- */
                         /*   hull pair's winning facet may be one qconvex's  */
                         /*   default pre-merge joins (LQRO_REC_QHMERGE_WIN): */
                         /*   this build restates Qhull merge-free, so that   */
                         /*   pair's facet, distance and half-plane are not   */
                         /*   pinned to the reference (LQRO:925-939, 956-967; */
                         /*   lqro_get_qhmerge_pairs names the pairs).        */
                         /*   LQRO_E_HULL takes precedence when both apply.   */
};

/* ---- flags ------------------------------------------------------------- */
#define LQRO_FLAG_RECORDS     0x1  /* keep per-pair records for lqro_get_records */
#define LQRO_FLAG_QHULL_ORDER 0x2  /* inside-hull branch with the reference's own rule   */
                                   /*   (LQRO:925-968): Qhull's facet order and each    */
                                   /*   facet's first Fv vertex, strict '<', and the    */
                                   /*   loop-carried normalVector when facet 0 wins     */
                                   /*   (LQRO:956-968, 1385); built in-kernel by k_qhull */

/* per-pair record flags (lqro_pair_record.flags) */
#define LQRO_REC_PLANE    0x01  /* n_reach > min_reach: a half-plane was emitted (LQRO:1409) */
#define LQRO_REC_INSIDE   0x02  /* GJK put vrel inside the hull (LQRO:855-864)          */
#define LQRO_REC_BACKUP   0x04  /* GJK took its backup procedure (GJK:663-706)          */
#define LQRO_REC_HULL     0x08  /* the in-kernel hull produced the plane (LQRO:867-969) */
#define LQRO_REC_HULLFAIL 0x10  /* hull degenerate / capacity exceeded                  */
#define LQRO_REC_LOCAL    0x20  /* the plane came from the local hull (k_lhull)          */
#define LQRO_REC_STALE    0x40  /* Qhull order: facet 0 won, normal = the loop-carried    */
                                /*   normalVector of the previous pair (LQRO:956-968)    */
#define LQRO_REC_QHMERGE  0x80  /* Qhull order: Qhull would merge facets in this hull;   */
                                /*   built merge-free                       */
#define LQRO_REC_QHMERGE_WIN 0x100 /* with LQRO_REC_QHMERGE: a facet within 1e-6 of the  */
                                /*   winning distance has another hull vertex within    */
                                /*   1e-9 (|coord|max + 1) of its plane, so qconvex's     */
                                /*   pre-merge may have joined the winner into a merged */
                                /*   facet: the pair's facet, distance and normal are    */
                                /*   then not pinned to the reference;    */
                                /*   lqro_get_stats_ex [11] counts these pairs           */

/* Static configuration.  The names follow the reference's compile-time
 * macros (LQRO:9-14) and the constants of its driver (LQRO:1387, 1224). */
typedef struct lqro_config {
  int32_t n_agents;      /* NUM_QUADS                                             */
  int32_t x_dim;         /* X_DIM (simulator2.h:4) — 16                           */
  int32_t u_dim;         /* U_DIM — 4                                             */
  int32_t horizon;       /* OBSTACLE_STEPS (LQRO:11)                              */
  int32_t n_points;      /* NUM_POINTS (LQRO:12) points per sampled ellipsoid     */
  int32_t min_reach;     /* pairs with n_reach <= min_reach emit no plane (4, LQRO:1409) */
  double  xy_radius;     /* XYRADIUS (LQRO:13); the sphere uses 2*XYRADIUS        */
  double  z_radius;      /* ZRADIUS  (LQRO:14)                                    */
                         /* a zero semi-axis (a flat set, a needle, a point) is
                          * accepted by the step and refused by the clearance
                          * calls (LQRO_E_ARG, see lqro_clearance)              */
  double  vmax_reach;    /* reachable-velocity radius, 30 (LQRO:1387)             */
  double  vmax_lp;       /* LP speed bound, 100 (LQRO:1224)                        */
  int32_t row_begin;     /* agents [row_begin,row_end) are this context's rows    */
  int32_t row_end;       /*   (multi-GPU sharding; 0,0 = all rows)                 */
  int32_t device;        /* HIP device ordinal                                    */
  int32_t flags;         /* LQRO_FLAG_*                                           */
  int32_t row_stride;    /* 0/1: rows row_begin..row_end-1; s > 1: rows row_begin,  */
                         /*   row_begin+s, ... < row_end (cyclic sharding: rank,  */
                         /*   world); records, newv rows and the LP follow it      */
} lqro_config;

/* Physical model + cost weights: the globals set by setup() and _tmain
 * (LQRO:169-189, 1275-1286, 559-561). */
typedef struct lqro_model {
  double dt, gravity, mass, inertia, moment_const, thrust_latency, length;
  double j_step;          /* central-difference step (LQRO:189)   */
  double qv, qp, r;       /* Qv = qv*I3, Qp = qp*I3, R = r*I4     */
  double pos_weight;      /* 0.05 in LQRO:559-561 (0.25 in PCW)   */
} lqro_model;

/* One record per ordered pair (i, j), j != i, kept when LQRO_FLAG_RECORDS
 * is set.  Field-for-field what the reference computes in LQRO:1401-1417. */
typedef struct lqro_pair_record {
  int32_t i, j;
  int32_t n_reach;        /* reachablePoints.size() (LQRO:1408)              */
  int32_t flags;          /* LQRO_REC_*                                      */
  int32_t gjk_iters;      /* G-tests performed by gjk_distance               */
  int32_t simplex_n;      /* final GJK simplex size                          */
  int32_t simplex[4];     /* final GJK simplex: indices into reachablePoints */
  int32_t facet[3];       /* hull branch: arg-min facet (reachable indices); */
                          /*   Qhull order: in Fv order, facet[0] = the vertex */
                          /*   the distance is measured from (LQRO:934-937)  */
  int32_t n_facets;       /* hull branch: number of hull facets (LQRO_REC_LOCAL: */
                          /*   the certified facets of the local hull)       */
  uint64_t reach_hash;    /* sum of splitmix64(q) over reachable point ids q */
  double dist;            /* distance before the *0.5 of LQRO:1416           */
  double normal[3];       /* normalVector fed to createHalfPlanes            */
  double wpt_vrel[3];     /* GJK witness on the vrel point                   */
  double wpt_hull[3];     /* GJK witness on the hull                         */
  float  plane_point[3];  /* Plane.point  (fp32, LQRO:1217-1219)             */
  float  plane_normal[3]; /* Plane.normal (fp32, LQRO:1210)                  */
} lqro_pair_record;

typedef struct lqro_ctx lqro_ctx;

/* Defaults: LQRO's constants (N given by the caller); flags =
 * LQRO_FLAG_QHULL_ORDER, the reference's own inside-hull rule.  Clearing it
 * selects the faster canonical facet rule, a measured deviation from the
 * reference. */
void lqro_config_default(lqro_config* cfg, int32_t n_agents, int32_t horizon, int32_t n_points);
void lqro_model_default(lqro_model* m);

/* Replaces controlMatrices (LQRO:520-582) and linearizeDiscretize (LQRO:456-471):
 * the velocity LQR (A,B,c,L,E) and the position LQR (Lh,Eh) at hover.
 * Host C++ (setup time, once per agent type).  Any out pointer may be NULL. */
int lqro_synthesize_gains(const lqro_model* m,
                          double* A  /* X*X */, double* B  /* X*U */, double* c /* X */,
                          double* L  /* U*X */, double* E  /* U*3 */,
                          double* Lh /* 3*X */, double* Eh /* 3*3 */);

/* The same synthesis for a swarm of heterogeneous agents, on the GPU (one
 * agent per lane): models[n]; outputs are n consecutive blocks of the shapes
 * above (A n*X*X, B n*X*U, c n*X, L n*U*X, E n*U*3, Lh n*3*X, Eh n*3*3), host
 * arrays, any may be NULL.  Bit-identical to lqro_synthesize_gains per model.
 * Feeds lqro_set_gains(..., per_agent = 1).  Synchronous. */
int lqro_synthesize_gains_batch(const lqro_model* models, int32_t n,
                                double* A, double* B, double* c, double* L, double* E,
                                double* Lh, double* Eh, int32_t device);

/* The same two syntheses for a state width x_dim: 16 (the reference's
 * quadrotor, identical to the two calls above) or 12, the reduced model of
 * BASELINE config 5: the 4 rotor-force states of X_DIM = 16
 * (simulator2.h:4) dropped, rotor forces = the command (no thrust lag), every
 * other term of f (LQRO:368-397) unchanged, linearised at the same hover
 * point.  Shapes as above with X = x_dim.  Both also return l (U), the
 * feedforward of controlMatrices (LQRO:552-557: pseudoInverse over jacobi2,
 * MAT:450-477, 887-1037), 0 at the reference's hover point (c = 0). */
int lqro_synthesize_gains_x(const lqro_model* m, int32_t x_dim,
                            double* A, double* B, double* c, double* L, double* E,
                            double* l /* U: the feedforward term, LQRO:552-557 */,
                            double* Lh, double* Eh);
int lqro_synthesize_gains_batch_x(const lqro_model* models, int32_t n, int32_t x_dim,
                                  double* A, double* B, double* c, double* L, double* E,
                                  double* l /* n*U */, double* Lh, double* Eh, int32_t device);

/* Replaces createSpheres (LQRO:735-750): NP Fibonacci-sphere points. */
int lqro_sphere(int32_t n_points, double xy_radius, double z_radius, double* out /* NP*3 */);

int  lqro_create(const lqro_config* cfg, lqro_ctx** out);
void lqro_destroy(lqro_ctx* ctx);

/* Gains read by the pair loop: A, B shared (LQRO:1265-1266, 1371); L_i, E_i
 * per agent (Quadrotor::L,E, LQRO:90-91).  per_agent = 0: one L,E for all
 * agents (the reference's case: every agent gets the same gains, LQRO:1371);
 * per_agent = 1: L is n_agents*U*X, E is n_agents*U*3.  Builds the per-agent
 * horizon tables on the device (findFG + createObstacle's Transform, LQRO:723-732,
 * 770-773). */
int lqro_set_gains(lqro_ctx* ctx, const double* A, const double* B,
                   const double* L, const double* E, int32_t per_agent);

/* Opt-in neighbour culling, in place of the all-pairs
 * loop (LQRO:1396): agent i then computes only the pairs with the
 * max_neighbors agents j != i of smallest |p_i - p_j|^2 < neighbor_dist^2
 * (ties to the lower j), RVO2-3D's computeNeighbors / insertAgentNeighbor
 * (Agent.cpp:74-81, 153-174) with agents visited in j order; its LP sees those
 * planes in j order.  A row then has K = min(max_neighbors, n_agents-1) slots
 * instead of n_agents-1: lqro_get_records returns rows x K records, the q-th
 * the row's q-th neighbour in ascending j; unused slots have j = -1 and
 * n_reach = -1.  lqro_get_stats()[0] counts the kept pairs.  This CHANGES
 * results against the reference.  max_neighbors <= 0 restores all pairs. */
int lqro_set_neighbors(lqro_ctx* ctx, double neighbor_dist, int32_t max_neighbors);

/* ---- opt-in constraints that are not agents ---------------------------
 * The reference's LP sees the N-1 pair planes only.  The three calls below
 * put extra half-planes AHEAD of them in each row's orcaPlanes_, the way
 * RVO2's Agent::computeNewVelocity puts its obstacle lines before the agent
 * lines of the same LP (Agent.cpp:84-151; there is no counterpart in LQRO).
 * Row agent i's plane list becomes: its fence planes (0..6), then its user
 * planes in the order given, then the pair planes exactly as before;
 * calculateNewV (LQRO:1223-1234) runs over that list unchanged.  A velocity
 * v satisfies a plane when normal.(v - point) >= 0, in the agent's absolute
 * velocity space (the LP's own convention, LQRO:1083).  Extra planes are as
 * soft as every other plane (linearProgram4 relaxes them like the rest)
 * unless lqro_set_hard_planes below makes them hard;
 * inputs must be finite.  Pair records, stats, the hull queue and the
 * carried normal do not see them.  All arrays are indexed by the global
 * agent id, so every row shard takes the same arrays and reads its own rows.
 * With nothing set the step is the reference's; once set, results CHANGE
 * against the reference.  Each call returns LQRO_E_STATE while a
 * lqro_step_device_begin is pending, and waits for the last enqueued step
 * before it replaces a buffer. */

/* User half-planes, host arrays (copied): agent i owns
 * planes[6*offsets[i] .. 6*offsets[i+1]), six floats a plane (point xyz,
 * normal xyz: lqro_calculate_new_v's layout); offsets has n_agents + 1
 * entries.  planes == NULL clears.  Decreasing offsets or more than 8192
 * planes for one agent: LQRO_E_ARG.  Stands in for RVO2's obstacle-first
 * plane order (AGT:84-151). */
int lqro_set_user_planes(lqro_ctx* ctx, const float* planes, const int64_t* offsets);

/* The same, device-resident at a fixed pitch: agent i's planes start at
 * d_planes + 6*max_per_agent*i and d_counts[i] <= max_per_agent of them are
 * live (d_counts == NULL: all; a count outside [0, max_per_agent] is
 * clamped).  The pointers are read when the row's LP runs: the caller keeps
 * them alive and writes them on the stream the step is enqueued on, before
 * the step — the path for planes that change every step.  max_per_agent <= 0
 * clears; above 8192: LQRO_E_ARG.  lqro_set_user_planes builds this layout
 * in buffers of the context's own.  Stands in for RVO2's obstacle-first
 * plane order (AGT:84-151). */
int lqro_set_user_planes_device(lqro_ctx* ctx, const float* d_planes, int32_t max_per_agent,
                                const int32_t* d_counts);

/* An axis-aligned box [lo, hi] the agents' ellipsoids should stay inside,
 * with time horizon tau seconds; stands in for RVO2's obstacle-first plane
 * order (AGT:84-151) with the box's faces as the obstacles.  Every step
 * writes, for each own row i, axis a = x, y, z in that order, first the
 * lower face, then the upper:
 *   lower: normal = +e_a, point[a] = (float)(((lo[a] + m[a]) - p[a]) / tau)
 *   upper: normal = -e_a, point[a] = (float)(((hi[a] - m[a]) - p[a]) / tau)
 * (the point's other components +0), p = x[i][0..2] of the step's x, m =
 * (xy_radius, xy_radius, z_radius); fp64 in exactly that order, rounded
 * once.  A face whose bound is +-infinity is not emitted (lo = (-inf, -inf,
 * 0), hi = +inf: a floor alone), so every agent has the same number of fence
 * planes.  tau <= 0 or lo/hi == NULL turns the fence off; lo[a] + 2 m[a] >
 * hi[a]: LQRO_E_ARG. */
int lqro_set_fence(lqro_ctx* ctx, const double lo[3], const double hi[3], double tau);

/* ---- obstacles: columns of the pair loop that are not agents -----------
 * The reference's loop was written to run its pipeline once more, after the
 * j loop, against a body that is no quadrotor (floorState / floorPoints,
 * LQRO:1377-1379 and the commented block LQRO:1421-1434: createObstacle, GJK /
 * convexHull, then createHalfPlanes WITHOUT the distance *= 0.5 of :1416,
 * before the row's calculateNewV).  These calls generalise that block to M
 * bodies: row agent i's pair loop visits the columns j = 0..n_agents-1, j != i
 * as before, then j = n_agents + o for obstacle o = 0..M-1, in that order.
 * An obstacle is one state of x_dim doubles ([0..2] position, [3..5]
 * velocity, the rest as the caller's model has them: hover attitude and
 * nominal rotor forces make x_i - x_o a position / velocity difference) and
 * is treated exactly as the reference treats "the other agent":
 * Translate_k = -C F_k (x_i - x_o) with the row agent's own tables, so a
 * moving obstacle is extrapolated like an agent holding its velocity.
 * Obstacles have no gains, no vgoal and never own a row.
 *   - responsibility in (0, 1] replaces the 0.5 of LQRO:1416 for an obstacle
 *     column (1.0: the agent does all the avoiding, LQRO:1434; 0.5: an
 *     obstacle column is bit-identical to an agent column);
 *   - the obstacle columns' point set is createSpheres (LQRO:735-750) with
 *     2*XYRADIUS replaced by (xy_radius + obs_xy_radius) and 2*ZRADIUS by
 *     (z_radius + obs_z_radius), the sum formed first: obstacle radii equal
 *     to the agents' give the agents' set bit for bit, radii (0, 0) give
 *     createFloorSpheres (LQRO:752-767), a point obstacle.  One shape and one
 *     responsibility for all the obstacles of these two calls
 *     (lqro_set_obstacles_ex below: one of each per obstacle).
 * A row then has n_agents - 1 + M slots: the loop-carried normalVector
 * (LQRO:1385) runs through the obstacle columns like through any pair, the
 * row's LP sees their planes after the agents' (fence and user planes stay
 * ahead), and records (j = n_agents + o), statistics, hull builds, hull
 * failures and merge suspects count them like pairs.  With lqro_set_neighbors
 * the obstacles are candidates like agents (K = min(max_neighbors, n_agents
 * + M - 1)).  Every row shard takes the same obstacles.  n_obstacles <= 0 or
 * a null pointer clears and returns the context to the sizes and state of
 * one that never had obstacles.  Radii negative or not finite, or a
 * responsibility outside (0, 1]: LQRO_E_ARG.  LQRO_E_STATE while a
 * lqro_step_device_begin is pending; waits for the last enqueued step before
 * it replaces a buffer.  Changing M renumbers the pair slots: what the
 * schedule kept per slot is reset, the carried normal stays.  With nothing
 * set the step is the reference's; once set, results CHANGE against the
 * reference. */
int lqro_set_obstacles(lqro_ctx* ctx, const double* states /* M*X, host, copied */, int32_t n_obstacles,
                       double obs_xy_radius, double obs_z_radius, double responsibility);
/* The same with the states device-resident: d_states is read when the step
 * runs, so the caller keeps it alive and writes it on the stream the step is
 * enqueued on, before the step — the path for obstacles that move every
 * step (lqro_set_user_planes_device's contract). */
int lqro_set_obstacles_device(lqro_ctx* ctx, const double* d_states /* M*X, read when the step runs */,
                              int32_t n_obstacles, double obs_xy_radius, double obs_z_radius,
                              double responsibility);
/* A shape and a responsibility per obstacle: a 0.3 m pole, a 5 m balloon
 * that cooperates at 0.5 and a piloted aircraft that never yields at 1.0 in
 * one scene.  The two calls above forward here with their three scalars
 * broadcast, and their results are unchanged bit for bit.
 *   - Point set.  Obstacle o's column uses createSpheres with (xy_radius +
 *     xy_radius[o]) and (z_radius + z_radius[o]), the sum formed first, as
 *     above.  NULL for either array: the agents' radii for every obstacle.
 *   - Factor.  distance *= responsibility[o] replaces the 0.5 of LQRO:1416 for
 *     that column.  NULL: 1.0 for every obstacle.
 *   - Classes.  Distinct shapes are found by comparing the generated point
 *     sets bit for bit.  A set equal to the agents' uses the agents' tables and
 *     costs nothing; the others are classes 1..K in order of first
 *     appearance, each with a point set, a slice bound and a block of k_pair's
 *     LDS of its own (3 n_points + horizon + 4 doubles).  More than
 *     LQRO_OBS_SHAPES_MAX classes: LQRO_E_ARG; so is a layout in which the
 *     class blocks leave no wave of k_pair its LDS region (large horizon x
 *     n_points), a radius negative or not finite and a responsibility outside
 *     (0, 1].  With no class of their own the LDS layout, its size and the wave
 *     count are those the context was created with.
 *   - Everything else is as above: the column order j = n_agents + o, the
 *     carried normal, records, statistics, hull failures and merge suspects,
 *     culling, shards, hard planes, clearing and renumbering, LQRO_E_STATE
 *     while a lqro_step_device_begin is pending; a failed call leaves the
 *     context as it was.
 *   - Culling.  lqro_set_neighbors ranks candidates by centre distance, the
 *     obstacles among them: with culling on, a large obstacle can be dropped
 *     from a row's list while its surface is near.  Give max_neighbors room for
 *     the obstacles in range, or leave culling off with large shapes.
 * The three arrays are host arrays of n_obstacles doubles, copied by both
 * calls; only the states of the _device call stay the caller's. */
#define LQRO_OBS_SHAPES_MAX 8
int lqro_set_obstacles_ex(lqro_ctx* ctx, const double* states /* M*X, host, copied */, int32_t n_obstacles,
                          const double* xy_radius /* M, host; NULL: the agents' */,
                          const double* z_radius /* M, host; NULL: the agents' */,
                          const double* responsibility /* M, host; NULL: all 1.0 */);
int lqro_set_obstacles_ex_device(lqro_ctx* ctx, const double* d_states /* M*X, read when the step runs */,
                                 int32_t n_obstacles, const double* xy_radius, const double* z_radius,
                                 const double* responsibility);

/* ---- hard planes: constraints linearProgram4 does not relax ------------
 * The fence, user and obstacle planes above are as soft as the pair planes:
 * once a row's list is infeasible, linearProgram4 (LQRO:1160-1206) gives way
 * on all of them alike.  RVO2 keeps its obstacle lines out of that
 * relaxation: its 2-D linearProgram3(lines, numObstLines, beginLine, ..)
 * copies the first numObstLines lines into every projected list as they are
 * and projects only the agent lines.  lqro_set_hard_planes carries that rule
 * to this LP.  The levels form a ladder, so the hard planes are always a
 * prefix of row i's list, n_hard of them:
 *   LQRO_HARD_NONE      none (the default: the step is as without this call)
 *   LQRO_HARD_FENCE     the row's fence planes
 *   LQRO_HARD_HEAD      its fence planes, then its live user planes
 *   LQRO_HARD_OBSTACLES fence, user, then its obstacle columns' planes, which
 *                       the LP then takes in column order o AHEAD of the
 *                       agent planes (fence, user, obstacles, agents); with
 *                       lqro_set_neighbors the obstacle slots are those whose
 *                       neighbour is a column >= n_agents, the last of the
 *                       row's kept slots.
 * n_hard counts the planes actually in the list (no face at infinity, the
 * clamped user count, no obstacle column without a plane).  linearProgram3
 * and calculateNewV are unchanged; in linearProgram4(planes, n_hard,
 * beginPlane, radius, result), for a violated plane i >= beginPlane,
 * projPlanes is planes[0 .. n_hard) copied as they are, followed by the
 * projections of planes j = n_hard .. i-1 computed as before (for i < n_hard
 * the projected part is empty and all n_hard planes are still copied, plane
 * i included, as in RVO2); the inner linearProgram3, the restore on failure
 * and the distance update are unchanged.  With n_hard = 0 the row's LP is the
 * reference's in every bit and every launch.
 * What this promises: once the hard planes and the speed sphere are feasible
 * together and the result satisfies them, no later relaxation leaves them.
 * What it does not: if linearProgram3 fails ON a hard plane, or the hard
 * planes are infeasible among themselves, the result is kept as RVO2 keeps
 * it, and nothing is guaranteed.
 * Only the LP's view moves at LQRO_HARD_OBSTACLES: records and their order,
 * statistics, the hull queue, the carried normal's (i, j) order and
 * LQRO_E_HULL / LQRO_E_QHMERGE are unchanged.  The level stays when fence,
 * user planes or obstacles are later set or cleared; every row shard takes
 * the same level.  A level outside 0..3: LQRO_E_ARG.  LQRO_E_STATE while a
 * lqro_step_device_begin is pending; waits for the last enqueued step before
 * it takes effect; allocates nothing.  Results CHANGE against the reference
 * once a row has a hard plane. */
#define LQRO_HARD_NONE      0
#define LQRO_HARD_FENCE     1
#define LQRO_HARD_HEAD      2
#define LQRO_HARD_OBSTACLES 3
int lqro_set_hard_planes(lqro_ctx* ctx, int32_t level);

/* ---- activity mask: agents that leave and rejoin the swarm ----------------
 * A context's swarm is n_agents bodies for its whole life; the mask says
 * which of them take part in a step.  The reference has no counterpart: its
 * NUM_QUADS is a compile-time constant (LQRO:9).  active[i] != 0: agent i
 * takes part; N bytes indexed by the global agent id (every row shard takes
 * the same array).  An inactive agent is neither a row nor a column of the
 * step: the step over N agents with mask a equals the step over the compacted
 * swarm x[a], vgoal[a], the per-agent tables [a] and the same obstacles, rows
 * and columns in their relative order.
 *   - Columns.  In an active row the slot of an inactive column holds no
 *     plane: its flag is written as 0 this step, whatever an earlier step left
 *     there.  The column adds no hull job, no hull-build record and nothing to
 *     the counters, and is never named by lqro_get_hull_failures or
 *     lqro_get_qhmerge_pairs.  Obstacle columns (j >= n_agents) are not masked.
 *   - Rows.  An inactive own row does no pair work and no LP and gets no fence
 *     or user planes; newv[3i..3i+2] is written as +0.0 by lqro_step,
 *     lqro_step_device and lqro_step_device_end alike; its entry of the
 *     n_agents x 4 row-normal table is that of a row without a plane.
 *   - The carried normal runs through the active pairs in (i, j) order; a step
 *     without an active pair leaves it as it entered.
 *   - Records (LQRO_FLAG_RECORDS): the count and the slot numbering do not
 *     change (slot q of row i is column q + (q >= i)); a slot whose row or
 *     column is inactive has i and j set and every other field zero.
 *   - lqro_get_stats()[0] counts the slots visited: for each active own row the
 *     active columns other than itself plus the obstacle columns (with
 *     lqro_set_neighbors the kept neighbours, as before).
 *   - Slot numbers do not move (unlike lqro_set_obstacles), so what the
 *     schedule keeps per slot stays valid; a pair it carried over from the last
 *     step whose row or column is now inactive is dropped at the head of the
 *     step, before anything is built for it.  The schedule is planned for
 *     n_agents whatever the mask (a device mask's count is known on the device
 *     only); results do not depend on it.
 *   - lqro_set_neighbors: inactive agents are no candidates; K stays
 *     min(max_neighbors, n_agents - 1 + M); an inactive row's list is all -1.
 *   - Clearance (the monitor and lqro_clearance[_device]): inactive agents are
 *     neither measured rows nor columns; an inactive own row's record is the
 *     cleared one (minima +inf, indices -1, n_hit 0, hit[] -1) and adds nothing
 *     to the totals.  The explicit calls read the mask when they run.
 *   - LP audit: an inactive own row's record is the cleared one (i set, m =
 *     n_hard = 0, maxima -inf with indices -1, counts 0, v2 = dv2 = 0) and the
 *     row is left out of every total, dv2_max included.
 *   - lqro_calculate_new_v*, lqro_audit_new_v and lqro_dynamics_step* take no
 *     context and do not see the mask.
 * NULL clears: the context is then the one that never had a mask, in every
 * launch, size and result; an all-ones mask gives bit-identical results too.
 * The host form copies the bytes.  The device form keeps the pointer: the
 * bytes are read on the step's stream when the step runs, so the caller keeps
 * them alive and may rewrite them there before every step
 * (lqro_set_obstacles_device's contract).  Both wait for the last enqueued
 * step, return LQRO_E_STATE while a lqro_step_device_begin is pending and
 * LQRO_E_ARG for a null context, allocate nothing inside a step, and leave the
 * context as it was when they fail.  The mask stays when obstacles, fence, user
 * planes, neighbours, hard planes, monitor or audit are set or cleared, and
 * setting it keeps all of those and the since-reset totals.  lqro_version()
 * does not change: callers detect the feature by the symbol. */
int lqro_set_active(lqro_ctx* ctx, const uint8_t* active /* N, host, copied */);
int lqro_set_active_device(lqro_ctx* ctx, const uint8_t* d_active /* N, read when the step runs */);

/* ---- interaction classes: who avoids whom, and by how much -----------------
 * Every agent belongs to one of n_classes classes (cls[i], N bytes indexed by
 * the global agent id; every row shard takes the same arrays), and
 * share[a * C + b], in [0, 1], is the factor a row of class a applies against
 * an AGENT column of class b in place of the reference's fixed 0.5
 * (LQRO:1416): one fp64 multiply of the pair's distance, rounded once,
 * wherever the step forms a half-plane.  The reference has no counterpart;
 * RVO-style libraries ship it as avoidance layers, masks and priorities.
 * 0.5 in every entry gives the step without a table, bit for bit;
 * share[a][b] + share[b][a] >= 1 (the two halves cover the whole avoidance) is
 * the caller's business and is not checked.
 *   - An ignored pair.  A share of exactly 0.0: row i ignores column j.  The
 *     slot is treated exactly as lqro_set_active treats an inactive column: no
 *     pair work, no hull job, its flag written as 0 this step, its record zero
 *     with i and j set; it adds nothing to the counters, is never named by
 *     lqro_get_hull_failures or lqro_get_qhmerge_pairs and never listed, marked
 *     or queued by the schedule.  Any share > 0.0 is live, however small.
 *   - A pair (i, j < n_agents) is live when row i is active, column j is
 *     active (lqro_set_active; the two compose) and share[cls[i]][cls[j]] > 0.
 *     Obstacle columns (j >= n_agents) do not see the table: they keep their
 *     own responsibility and are never ignored.
 *   - A row whose every agent column is ignored is still a row: it gets its
 *     fence, user and obstacle planes and its LP runs (without a plane the LP
 *     returns vgoal clipped to vmax_lp), unlike an inactive row (newv +0.0).
 *   - The carried normal runs through the live pairs in (i, j) order, and the
 *     n_agents x 4 row-normal table follows; a step without a live pair leaves
 *     the carry as it entered.
 *   - lqro_get_stats()[0] counts the live slots: for each active own row i the
 *     active agents of every class b with share[cls[i]][b] > 0, less 1 when
 *     share[cls[i]][cls[i]] > 0 (itself), plus the obstacle columns (with
 *     lqro_set_neighbors the kept neighbours, as before).
 *   - lqro_set_neighbors: a column row i ignores is no candidate of row i and
 *     uses up none of its K slots; K does not change.
 *   - Slot numbers and the record count do not move.  Clearance and prediction
 *     (monitor and explicit calls) do not see the table: they measure bodies,
 *     not intentions.  The LP audit follows the slots' flags as ever; the
 *     hard-plane levels are unchanged.  lqro_calculate_new_v*, lqro_audit_new_v
 *     and lqro_dynamics_step* take no context and do not see it.
 * cls == NULL or share == NULL clears: the context is then the one that never
 * had a table, in every launch, size and result.  The share table is copied by
 * both forms.  The host form checks and copies the class bytes; the device
 * form keeps the pointer: the bytes are read on the step's stream when the step
 * runs, so the caller keeps them alive and may rewrite them there before every
 * step (lqro_set_active_device's contract); a device byte >= n_classes is read
 * as n_classes - 1.  LQRO_E_ARG: a null context, n_classes outside
 * 1..LQRO_CLASSES_MAX, a share outside [0, 1] or not finite, a host class byte
 * >= n_classes.  Both wait for the last enqueued step, return LQRO_E_STATE
 * while a lqro_step_device_begin is pending, allocate nothing inside a step,
 * and leave the context as it was when they fail.  The table stays when the
 * mask, obstacles, fence, user planes, neighbours, hard planes, monitor or
 * audit are set or cleared, and setting it keeps all of those and the
 * since-reset totals.  lqro_version() does not change: callers detect the
 * feature by the symbol. */
#define LQRO_CLASSES_MAX 16
int lqro_set_interaction(lqro_ctx* ctx, const uint8_t* cls /* N, host, copied */,
                         int32_t n_classes, const double* share /* C*C, host, copied */);
int lqro_set_interaction_device(lqro_ctx* ctx, const uint8_t* d_cls /* N, read when the step runs */,
                                int32_t n_classes, const double* share /* C*C, host, copied */);

/* One control step: the pair loop LQRO:1393-1436 for the context's rows.
 * x: n_agents*X agent states (Quadrotor::x), vgoal: n_agents*3,
 * newv: n_agents*3 (only rows [row_begin,row_end) are written).  Host
 * pointers; blocks until newv is ready.  Returns LQRO_E_HULL (newv still
 * written) when an inside-hull pair got no half-plane, else LQRO_E_QHMERGE
 * (newv written) when an inside-hull pair's winner may be a facet qconvex
 * merges (LQRO_REC_QHMERGE_WIN). */
int lqro_step(lqro_ctx* ctx, const double* x, const double* vgoal, double* newv);

/* Same, device-resident: d_x, d_vgoal, d_newv are device pointers on the
 * context's device; the work is enqueued on `stream` (hipStream_t; NULL = the
 * default null stream, as in lqro_dynamics_step_device) behind whatever the
 * caller queued there before, and the call returns without synchronising.
 * lqro_get_stats / lqro_get_records / lqro_get_timings wait for the last
 * enqueued step on the stream it was enqueued on.  The hull queue holds one
 * entry per pair slot, so a step cannot overflow it. */
int lqro_step_device(lqro_ctx* ctx, const double* d_x, const double* d_vgoal,
                     double* d_newv, void* stream);
/* (The device-resident calls cannot report a hull failure when they return:
 * lqro_get_stats()[4] / lqro_get_hull_failures after the step do, and
 * lqro_get_stats_ex()[11] / lqro_get_qhmerge_pairs the merge suspects.  While a
 * lqro_step_device_begin is pending, every call but lqro_step_device_end
 * returns LQRO_E_STATE.) */

/* lqro_step_device in two halves around the exchange a row-sharded caller
 * needs in Qhull order (LQRO_FLAG_QHULL_ORDER): the loop-carried
 * normalVector (LQRO:1385) runs through every pair of the swarm in (i, j)
 * order, across the shards.  _begin enqueues the sweep and the hulls and
 * writes, for each of the context's own rows i, the normal of its last pair
 * with one: d_rowtab[4 i + 0..2], d_rowtab[4 i + 3] = 1 (0 0 0 0 for none, or
 * without the flag).  The caller then fills the other ranks' rows of the
 * n_agents x 4 table (an all-gather) and calls _end, which resolves the
 * facet-0 pairs from the whole table (their own row's earlier pairs, else
 * the last row before theirs with a normal, else the normal entering the
 * step), runs the LP and writes d_newv.  Every rank then carries the same
 * normal into the next step.  For a context that owns every row the two
 * halves equal lqro_step_device.  lqro_step / lqro_step_device on a shard
 * other than the first resolve facet-0 pairs from the context's own rows
 * only. */
int lqro_step_device_begin(lqro_ctx* ctx, const double* d_x, const double* d_vgoal,
                           double* d_rowtab, void* stream);
int lqro_step_device_end(lqro_ctx* ctx, const double* d_rowtab, double* d_newv, void* stream);

/* calculateNewV (LQRO:1223-1234) for a batch of independent agents on the
 * GPU: agent r's planes are planes[offsets[r] .. offsets[r+1]) (6 floats
 * each: point xyz, normal xyz, in orcaPlanes_ push order), its preferred
 * velocity vgoal[3r..3r+2]; writes newv[3r..3r+2].  Synchronous. */
int lqro_calculate_new_v(const float* planes, const int64_t* offsets, int32_t n_agents,
                         const double* vgoal, double vmax_lp, double* newv, int32_t device);
/* The same with a hard prefix per agent (lqro_set_hard_planes' rule):
 * agent r's first n_hard[r] planes are kept out of linearProgram4's
 * relaxation.  n_hard[r] above the agent's plane count is clamped to it; a
 * negative value: LQRO_E_ARG; n_hard == NULL: all 0, which is
 * lqro_calculate_new_v. */
int lqro_calculate_new_v_hard(const float* planes, const int64_t* offsets, const int32_t* n_hard,
                              int32_t n_agents, const double* vgoal, double vmax_lp, double* newv,
                              int32_t device);

/* LQRO_FLAG_QHULL_ORDER: the loop-carried normalVector (LQRO:1385) entering
 * the context's first row (set; 0,0,0 at creation) and leaving its last
 * eligible pair after the last step (get).  A single context carries it
 * from step to step itself; row-sharded callers chain ranks with these. */
int lqro_set_carry_normal(lqro_ctx* ctx, const double* n3);
int lqro_get_carry_normal(lqro_ctx* ctx, double* n3);

/* Per-pair records of the last step (LQRO_FLAG_RECORDS): rows
 * [row_begin,row_end) x (n_agents-1) neighbours in j order, then the row's
 * obstacle columns (lqro_set_obstacles: j = n_agents + o). */
int lqro_get_records(lqro_ctx* ctx, lqro_pair_record* out, int64_t capacity, int64_t* n_out);

/* Counters of the last step: [0]=pairs, [1]=planes, [2]=inside, [3]=hull ok,
 * [4]=hull fail, [5]=gjk backups, [6]=sum n_reach, [7]=sum G-tests. */
int lqro_get_stats(lqro_ctx* ctx, int64_t* stats8);
/* The same counters and n - 8 more (n <= 12; words past 11 read 0):
 * [8] LQRO_FLAG_QHULL_ORDER hulls in which Qhull would merge facets
 *     (LQRO_REC_QHMERGE: built merge-free);
 * [9] builds k_qhull's per-insertion caps handed to k_qhull_big;
 * [10] of those, the ones a wave handshake timeout stopped;
 * [11] pairs whose winning facet qconvex's pre-merge may have merged
 *     (LQRO_REC_QHMERGE_WIN). */
int lqro_get_stats_ex(lqro_ctx* ctx, int64_t* stats, int32_t n);

/* The inside-hull pairs of the last step flagged LQRO_REC_QHMERGE_WIN (stats
 * [11]; lqro_step then returns LQRO_E_QHMERGE): *n_out = their number;
 * pairs[2k], pairs[2k+1] = (i, j) of the first min(*n_out, 64, capacity).
 * Replaces nothing in the reference: it names the pairs whose half-plane
 * may differ from convexHull's over a merged qconvex facet (LQRO:925-967). */
int lqro_get_qhmerge_pairs(lqro_ctx* ctx, int64_t* pairs, int64_t capacity, int64_t* n_out);

/* One Qhull-order hull build of the last step (LQRO_FLAG_QHULL_ORDER): the
 * in-kernel replacement of convexHull's qconvex run (LQRO:867-969) for the
 * pair (i, j), timed on the GPU's constant 100 MHz clock (s_memrealtime,
 * shared by every CU): from taking the job (the pair's points are computed
 * first) to its half-plane.  kernel: 0 k_qhull, 1 k_qhull_big (the build
 * beyond k_qhull's caps), 2 a k_qhull build handed to k_qhull_big (its
 * record ends where the hand-over happened). */
typedef struct lqro_hull_build {
  int32_t i, j;
  int32_t n_points;       /* reachablePoints.size(), qconvex's input             */
  int32_t insertions;     /* points Qhull added (qh_addpoint calls)              */
  int32_t facet_slots;    /* facets created (slots used)                         */
  int32_t kernel;
  uint64_t t_start, t_end;  /* 100 MHz ticks                                     */
} lqro_hull_build;
/* *n_out = the builds of the last step (at most the first `capacity` and
 * 16384 are written, in completion order). */
int lqro_get_hull_builds(lqro_ctx* ctx, lqro_hull_build* out, int64_t capacity, int64_t* n_out);

/* The pairs of the last step left without a half-plane because their hull
 * could not be built — degenerate input or every hull kernel's capacity
 * exceeded (stats [4]; lqro_step then returns
 * LQRO_E_HULL, the reference's qconvex always returns a hull, LQRO:879-880):
 * *n_out = their number; pairs[2k], pairs[2k+1] = (i, j) of the first
 * min(*n_out, 64, capacity). */
int lqro_get_hull_failures(lqro_ctx* ctx, int64_t* pairs, int64_t capacity, int64_t* n_out);

/* Device time of the kernels of the last step, ms, measured with HIP events on
 * the context's stream: [0]=pair sweep+GJK, [1]=hull, [2]=LP, [3]=whole step. */
int lqro_get_timings(lqro_ctx* ctx, float* ms4);

/* ---- clearance: did the swarm stay clear of anything? -------------------
 * An opt-in measurement, on the device, of each own row agent i against
 * every column: the agents c != i, then the obstacle columns n_agents + o of
 * lqro_set_obstacles[_ex] as the step reads them.  The reference has no
 * counterpart (its loop never asks); the body model is the method's own,
 * createSpheres over the summed radii (LQRO:735-750): column c's ellipsoid
 * has the semi-axes a_c = xy_radius + rxy_c, b_c = z_radius + rz_c, with
 * (rxy_c, rz_c) the configuration's radii for an agent column (a_c is the
 * reference's 2*XYRADIUS bit for bit) and the obstacle's own for an obstacle.
 * The host forms wxy_c = 1.0 / (a_c a_c), wz_c = 1.0 / (b_c b_c) once; then,
 * with p = x[.][0..2], all fp64 and every operation rounded once:
 *   dx = p_i.x - p_c.x (dy, dz likewise); q = dx dx + dy dy; d2 = q + dz dz;
 *   s2 = q wxy_c + (dz dz) wz_c;  the pair is a HIT when s2 < 1.0, strictly.
 * Self is skipped by index, never by distance (two agents at one point are a
 * hit with s2 == 0).  lqro_set_neighbors does not apply: every column counts.
 * Columns are numbered 0 .. n_agents + M - 1.  With lqro_set_fence active a
 * row's fence margin is the minimum over the emitted faces of
 *   lower face, axis a:  p[a] - (lo[a] + m[a])      (face index 2 a)
 *   upper face, axis a:  (hi[a] - m[a]) - p[a]      (face index 2 a + 1)
 * m = (xy_radius, xy_radius, z_radius): the fence planes' own expression
 * without the division by tau, the sign turned; the lowest face index wins a
 * tie; the row is OUT when the margin is < 0 (on a face, 0.0, is not out).
 * Inputs must be finite.  The result is deterministic: minima are taken over
 * (value, index) keys, counts are integers, no floating-point atomics; it
 * does not depend on schedule or wave count, and a numpy restatement
 * (tests/clearance_ref.py) matches it bit for bit. */
typedef struct lqro_clearance_row {
  double s2_min;       /* smallest s2 over the columns (+inf: no columns)         */
  double d2_min;       /* smallest d2 over the columns (+inf: no columns)         */
  double fence_min;    /* the fence margin; +inf without a fence                  */
  int32_t j_s2;        /* column of s2_min: the smallest on equal values; -1: none */
  int32_t j_d2;        /* column of d2_min, same tie rule                         */
  int32_t n_hit;       /* hit columns of this row: the true count, even past six  */
  int32_t fence_face;  /* the face 2 a + side that attains fence_min; -1: no fence */
  int32_t hit[6];      /* the first six hit columns, ascending, -1 padded         */
} lqro_clearance_row;

/* Over a context's own rows.  Ties: the smallest (value, i, j) wins.  n_hit
 * counts ordered pairs over the own rows: a context that owns every row
 * counts a touching agent pair twice, an agent-obstacle pair once.  A
 * minimum that is +inf (fence_min without a fence) has indices -1. */
typedef struct lqro_clearance_total {
  double s2_min, d2_min, fence_min;
  int32_t s2_i, s2_j;          /* the pair of s2_min                              */
  int32_t d2_i, d2_j;          /* the pair of d2_min                              */
  int32_t fence_i, fence_face; /* the row and face of fence_min                   */
  int64_t n_hit;               /* sum of the rows' n_hit                          */
  int64_t n_rows_hit;          /* rows with n_hit > 0                             */
  int64_t n_fence_out;         /* rows with fence_min < 0                         */
  int64_t n_measured;          /* measurements folded in (1 for a last total)     */
} lqro_clearance_total;
#ifdef __cplusplus
static_assert(sizeof(lqro_clearance_row) == 64, "lqro_clearance_row is 64 bytes");
static_assert(sizeof(lqro_clearance_total) == 80, "lqro_clearance_total is 80 bytes");
#endif

/* The context keeps two totals on the device: LAST, the last measurement
 * (n_measured = 1), and SINCE RESET, minima of minima and sums of counts over
 * every measurement since the last reset, its (i, j) those of the earliest
 * measurement that attains the minimum.  Explicit calls and the per-step
 * monitor both update them.  A row shard measures its own rows against all
 * columns; the caller merges the ranks' totals (min and sum with the tie
 * rules above: lqro.py merge_clearance; lqro::ShardedSimulator does not).
 * All calls: LQRO_E_ARG for a configuration whose xy_radius or z_radius is
 * not positive and finite; LQRO_E_STATE from lqro_clearance[_device] and
 * lqro_set_monitor while a lqro_step_device_begin is pending.  The buffers
 * are allocated by the first call that needs them, after the last step, and
 * never inside a step; lqro_set_obstacles* and lqro_set_fence keep the
 * monitor setting and the since-reset total. */

/* Measures the N x X host array x (the estimates or a caller's xTrue): copies
 * in, measures, waits, copies out.  rows: the context's own rows in row
 * order (NULL: not wanted); total: this measurement's (NULL: not wanted). */
int lqro_clearance(lqro_ctx* ctx, const double* x /* N*X, host */, lqro_clearance_row* rows /* nrows, may be NULL */,
                   lqro_clearance_total* total /* may be NULL */);
/* The same on a device array, asynchronous on the caller's stream (NULL: the
 * null stream, as in lqro_step_device), ordered behind the context's last
 * step and last measurement by event waits on that stream; once the buffers
 * exist it never waits on the host.  d_rows NULL: the context's own row
 * buffer; else the caller's nrows records, which lqro_get_monitor_rows /
 * _pairs then read: keep them alive until the next measurement. */
int lqro_clearance_device(lqro_ctx* ctx, const double* d_x, lqro_clearance_row* d_rows, void* stream);
/* on = 1: every lqro_step, lqro_step_device and lqro_step_device_begin
 * measures its own columns (the step's x and the obstacle states it reads) at
 * the head of the step, on the step's stream.  Nothing in the step reads the
 * result: newV, records, statistics and the carried normal are bit-identical
 * to a context without the monitor.  on = 0 (the default): no launch, no
 * buffer use.  Another value: LQRO_E_ARG. */
int lqro_set_monitor(lqro_ctx* ctx, int32_t on);
/* Waits for the last step or measurement (like lqro_get_stats), then copies
 * the two totals (either may be NULL); reset != 0 clears the since-reset
 * total after reading it.  A context that never measured: both cleared
 * (minima +inf, indices -1, counts 0). */
int lqro_get_monitor(lqro_ctx* ctx, lqro_clearance_total* last, lqro_clearance_total* since_reset, int32_t reset);
/* The last measurement's rows (capacity < the own rows: LQRO_E_ARG; no
 * measurement yet: *n_out = 0). */
int lqro_get_monitor_rows(lqro_ctx* ctx, lqro_clearance_row* rows, int64_t capacity, int64_t* n_out);
/* The last measurement's hit pairs (i, column) in (i, column) order, two
 * words a pair, assembled on the host from the rows' hit[]: at most six from
 * one row, so compare *n_out, the number written (at most capacity), with
 * the total's n_hit. */
int lqro_get_monitor_pairs(lqro_ctx* ctx, int64_t* pairs /* 2 per pair */, int64_t capacity, int64_t* n_out);

/* ---- horizon conflict prediction: each row's first predicted collision ----
 * An opt-in measurement, on the device: with the velocities v the step chose
 * (or any other N x 3 array), does the closed loop the LQR-obstacle was built
 * from keep each pair apart over the horizon, and if not, when and with whom
 * does it first fail?  The reference has no counterpart.  All fp64, every
 * operation rounded once, sums taken in ascending index order starting from
 * 0.0; no division and no sqrt on the device.
 * Tables.  For each gains set g (one, or N with per-agent gains) the step's
 * own recursion in its order: At = A + (B L), Bt = B E, G <- 0, then H times
 *   G <- (sum_m At[r][m] G[m][c]) + Bt[r][c];
 * CG_k is rows 0..2 of G after update k + 1, k = 0 .. H-1: slice k is the
 * state k + 1 steps ahead, the index of the step's T_k and NCF_k = -C F_k.
 * Path of a body b under set g with commanded velocity v_b, r = 0..2:
 *   P_b,k[r] = (sum_{c<3} CG_k[r][c] v_b[c]) - (sum_{m<X} NCF_k[r][m] x_b[m]).
 * An agent is predicted with its OWN set (with shared gains this equals the
 * step's model C F_k (x_i - x_j) + C G_k (v_i - v_j) in exact arithmetic).  An
 * obstacle has no gains: in row i it is predicted with ROW i's tables and
 * v_o = x_o[3..5], as the step treats it.  The affine terms c and l of the
 * closed loop are left out, as the method leaves them out.
 * Pair (own row i, column c, slice k).  Columns are the agents c != i, then
 * the obstacle columns n_agents + o, as in lqro_clearance.  With
 * d = P_i,k - P_c,k per component:
 *   q = dx dx + dy dy;  d2 = q + dz dz;  s2 = q wxy_c + (dz dz) wz_c
 * with lqro_clearance's host-formed weights over the summed radii; a HIT is
 * s2 < 1.0, strictly.  Self is skipped by index.  lqro_set_neighbors does not
 * apply.  With lqro_set_active (the caller's bytes, read when the measurement
 * runs) an inactive agent is neither a row nor a column; its row gets the
 * cleared record.  Obstacle columns are never masked.  Inputs must be finite.
 * Deterministic by construction: (value, index) keys, integer counts, no
 * floating-point atomics, no dependence on tile size, wave count or
 * schedule; a numpy restatement (tests/predict_ref.py) matches bit for bit.
 * Indices are -1 and minima +inf where nothing was measured. */
#define LQRO_PREDICT_TILE 8   /* own rows a workgroup of the pair kernel (no part of the result) */
typedef struct lqro_predict_row {
  double s2_min, d2_min;    /* over the columns and slices                               */
  int32_t j_s2, k_s2;       /* column and slice of s2_min: the smallest (value, column, slice) wins */
  int32_t j_d2, k_d2;       /* of d2_min, same rule                                      */
  int32_t k_first, j_first; /* the smallest slice with a hit; the smallest column hit at that slice */
  int32_t n_conf;           /* columns with a hit at any slice: the true count           */
  int32_t reserved;         /* 0                                                         */
  int32_t conf[4];          /* the first four conflict columns, ascending, -1 padded     */
} lqro_predict_row;

/* Over a context's own rows.  s2 / d2: the smallest (value, i, j, k) wins;
 * first: the smallest (k, i, j).  n_conf counts ordered (row, column) pairs. */
typedef struct lqro_predict_total {
  double s2_min, d2_min;
  int32_t s2_i, s2_j, s2_k, d2_i, d2_j, d2_k;
  int32_t first_k, first_i, first_j, reserved;
  int64_t n_conf;           /* sum of the rows' n_conf                                   */
  int64_t n_rows_conf;      /* rows with n_conf > 0                                      */
  int64_t n_measured;       /* measurements folded in (1 for a last total)               */
} lqro_predict_total;
#ifdef __cplusplus
static_assert(sizeof(lqro_predict_row) == 64, "lqro_predict_row is 64 bytes");
static_assert(sizeof(lqro_predict_total) == 80, "lqro_predict_total is 80 bytes");
#endif

/* The context keeps two totals on the device, LAST and SINCE RESET (minima
 * of minima, sums of counts; a strictly smaller value replaces the kept one,
 * so the indices are those of the earliest measurement attaining it).  A row
 * shard measures its own rows against all columns; the caller merges the
 * ranks' totals (lqro.py merge_prediction; lqro::ShardedSimulator does not).
 * There is no hook inside lqro_step: a row shard does not hold the other
 * rows' newV, so the hosts call these entry points.  Errors: LQRO_E_ARG for
 * NULL inputs and radii that are not positive and finite; LQRO_E_STATE while
 * a lqro_step_device_begin is pending and, for lqro_predict[_device], before
 * lqro_set_gains.  Buffers come from the context's pool at the first call
 * that needs them, after the last step and never inside one; lqro_set_gains
 * only marks the CG table stale (the next predicting call rebuilds it);
 * lqro_set_obstacles* resizes the buffers before its swap. */

/* Predicts from the host arrays x (N x X) and v (N x 3) and waits.  rows: the
 * context's own rows in row order (NULL: not wanted); total: this
 * measurement's (NULL: not wanted). */
int lqro_predict(lqro_ctx* ctx, const double* x, const double* v, lqro_predict_row* rows, lqro_predict_total* total);
/* The same on device arrays, asynchronous on the caller's stream, ordered
 * behind the context's last step and last measurement by event waits; once
 * the buffers exist it never waits on the host.  d_rows NULL: the context's
 * own row buffer (lqro_clearance_device's rules). */
int lqro_predict_device(lqro_ctx* ctx, const double* d_x, const double* d_v, lqro_predict_row* d_rows, void* stream);
/* The same measurement over caller-given paths [(N + M)][H][3] (an external
 * planner's trajectories): the M obstacle columns are the caller's own and
 * are treated as plain columns with the obstacle columns' weights. */
int lqro_predict_paths(lqro_ctx* ctx, const double* paths, lqro_predict_row* rows, lqro_predict_total* total);
int lqro_predict_paths_device(lqro_ctx* ctx, const double* d_paths, lqro_predict_row* d_rows, void* stream);
/* As lqro_get_monitor and lqro_get_monitor_rows. */
int lqro_get_prediction(lqro_ctx* ctx, lqro_predict_total* last, lqro_predict_total* since_reset, int32_t reset);
int lqro_get_prediction_rows(lqro_ctx* ctx, lqro_predict_row* rows, int64_t capacity, int64_t* n_out);
/* The agents' paths of the last lqro_predict[_device] as [agent][k][3];
 * LQRO_E_STATE when the last measurement used given paths or there is none. */
int lqro_get_paths(lqro_ctx* ctx, double* out /* N*H*3 */);

/* ---- LP audit: what did the LP do with each row's planes? ---------------
 * An opt-in measurement, on the device, of the step's result against the
 * plane list each own row's LP saw.  The reference has no counterpart.  For
 * own row agent i the list is, in this order: the emitted fence faces, the
 * live user planes (the count clamped to [0, max_per_agent]), then the pair
 * slots that hold a plane ([6] == 1) in slot order; at LQRO_HARD_OBSTACLES
 * with obstacles the obstacle slots come first and the agent slots after
 * (with lqro_set_neighbors the obstacle slots are the entries >= n_agents - 1
 * of the row's neighbour list).  k is a plane's index in that list, m the
 * list's length, n_hard the hard prefix the LP used.  With
 *   v = ((float)newv[3i], (float)newv[3i+1], (float)newv[3i+2]), the step's
 *   result, and pref = (float)vgoal[3i..],
 * all fp32, every operation rounded once, no contraction:
 *   viol_k = n.x (p.x - v.x) + n.y (p.y - v.y) + n.z (p.z - v.z), summed left
 *            to right: the LP's own violation expression (LQRO:1083, 1138,
 *            1170); plane k is violated when viol_k > 0
 *   v2  = v.x v.x + v.y v.y + v.z v.z
 *   dv2 = d.x d.x + d.y d.y + d.z d.z, d = v - pref
 * Ties: values compare as fp32 (+0 equals -0); of equal values the lowest k
 * wins.  kind / id name a plane's source:
 *   LQRO_AUDIT_FENCE   id = the face 2 a + side, numbered as in the clearance
 *                      measurement (the real face, not the emitted position)
 *   LQRO_AUDIT_USER    id = the index among the agent's user planes
 *   LQRO_AUDIT_COLUMN  id = the column j: an agent, or n_agents + o (without
 *                      lqro_set_neighbors slot q of row i is column
 *                      q + (q >= i); with it, the column of the neighbour
 *                      list's entry)
 * tol is the caller's tolerance, >= 0 (RVO_EPSILON, 0.00001f, suits a result
 * the LP reports as feasible).  Inputs must be finite.  The result is
 * deterministic: (value, k) keys and integer counts, no floating-point
 * atomics, no dependence on schedule or wave count; a numpy restatement
 * (tests/lp_audit_ref.py) matches it bit for bit. */
enum { LQRO_AUDIT_FENCE = 0, LQRO_AUDIT_USER = 1, LQRO_AUDIT_COLUMN = 2 };

typedef struct lqro_lp_row {
  float viol_max;       /* largest viol_k over the list; -inf for an empty list         */
  float hard_viol_max;  /* largest viol_k over k < n_hard; -inf when n_hard == 0        */
  float v2, dv2;        /* |v|^2 and |v - pref|^2                                       */
  int32_t i;            /* the row's global agent id                                    */
  int32_t m, n_hard;    /* the list's length and its hard prefix                        */
  int32_t n_viol;       /* planes with viol_k > 0.0f (linearProgram3's own test)        */
  int32_t n_viol_tol;   /* planes with viol_k > tol                                     */
  int32_t n_hard_viol;  /* planes k < n_hard with viol_k > tol                          */
  int32_t k_viol, kind_viol, id_viol;   /* the plane of viol_max; -1, -1, -1: empty list */
  int32_t k_hard, kind_hard, id_hard;   /* the plane of hard_viol_max; -1s: n_hard == 0  */
} lqro_lp_row;

/* Over a context's own rows.  A maximum is decided by the largest value, then
 * the smallest i, then the smallest k; a -inf maximum has indices -1. */
typedef struct lqro_lp_total {
  float viol_max;
  int32_t viol_i, viol_k, viol_kind, viol_id;
  float hard_viol_max;
  int32_t hard_i, hard_k, hard_kind, hard_id;
  float dv2_max;
  int32_t dv2_i;
  int64_t n_rows_viol;       /* rows with n_viol_tol > 0                        */
  int64_t n_rows_hard_viol;  /* rows with n_hard_viol > 0                       */
  int64_t n_viol_tol;        /* sum of the rows' n_viol_tol                     */
  int64_t n_planes;          /* sum of the rows' m                              */
  int64_t n_measured;        /* audits folded in (1 for a last total)           */
} lqro_lp_total;
#ifdef __cplusplus
static_assert(sizeof(lqro_lp_row) == 64, "lqro_lp_row is 64 bytes");
static_assert(sizeof(lqro_lp_total) == 88, "lqro_lp_total is 88 bytes");
#endif

/* on = 1: every lqro_step, lqro_step_device and lqro_step_device_end audits
 * its own rows at the end of the step, on the step's stream, behind the LP
 * (and the copy of the rows an early LP ran), reading the caller's d_newv.
 * Nothing in the step reads the result: newV, records, statistics and the
 * carried normal are bit-identical to a context without the audit.  The
 * context keeps two totals on the device: LAST (n_measured = 1) and SINCE
 * RESET, maxima of maxima (a strictly larger value replaces the kept one, so
 * the indices are those of the earliest step attaining it) and sums of counts.
 * on = 0 (the default): no launch, no buffer.  The buffers come from the
 * context's pool inside this call, after it has waited for the last step, and
 * never in a step.  LQRO_E_ARG: on outside {0, 1}, tol negative or not
 * finite; LQRO_E_STATE while a lqro_step_device_begin is pending.  The fence,
 * user-plane, obstacle, neighbour and hard-plane setters keep the setting and
 * the since-reset total.  A row shard audits its own rows; the caller merges
 * the ranks' totals (lqro.py merge_lp_audit; lqro::ShardedSimulator does not). */
int lqro_set_lp_audit(lqro_ctx* ctx, int32_t on, float tol);
/* Waits for the last step (like lqro_get_stats), then copies the two totals
 * (either may be NULL); reset != 0 clears the since-reset total after reading
 * it.  A context that never audited: both cleared (maxima -inf, indices -1,
 * counts 0). */
int lqro_get_lp_audit(lqro_ctx* ctx, lqro_lp_total* last, lqro_lp_total* since_reset, int32_t reset);
/* The last audit's rows, in own-row order (capacity < the own rows:
 * LQRO_E_ARG; no audit yet: *n_out = 0). */
int lqro_get_lp_audit_rows(lqro_ctx* ctx, lqro_lp_row* rows, int64_t capacity, int64_t* n_out);
/* Without a context, lqro_calculate_new_v_hard's twin: audits newv (n_agents
 * x 3) against the same plane lists (agent r's planes are planes[6 k ..] for
 * k in [offsets[r], offsets[r+1]), its first n_hard[r] hard, clamped to the
 * list's length; n_hard NULL: none), with the same two kernels.  Every plane
 * has kind LQRO_AUDIT_USER and id = k.  Synchronous.  rows (n_agents) and
 * total may be NULL. */
int lqro_audit_new_v(const float* planes, const int64_t* offsets, const int32_t* n_hard /* may be NULL */,
                     int32_t n_agents, const double* vgoal, const double* newv, float tol,
                     lqro_lp_row* rows /* may be NULL */, lqro_lp_total* total /* may be NULL */, int32_t device);

/* ---- the per-agent step after the pair loop ------
 * Replaces the agent loop LQRO:1437-1446: vGoal = newV; u = findU()
 * (riccatiControllerSteady, LQRO:594-617); propagateU (propagate,
 * LQRO:473-486) of the true state; kalmanFilter1 (LQRO:488-505); the
 * observation z = sampleGaussian(h(xTrue, RotTrue), N) (LQRO:1442);
 * kalmanFilter2 (LQRO:507-518); vGoal = findVGoal()
 * (riccatiControllerSteadyPosition, LQRO:619-645).  Quadrotor::visualize
 * (LQRO:1444) becomes a keyframe record instead of Callisto calls
 * (SURVEY §8f next #4).  X = 16, U = 4, Z = 6.
 * The reference draws its noise from rand() in agent order (normal(),
 * LQRO:334-350): the caller supplies the draws, LQRO_NORMALS_PER_AGENT per
 * agent (16 for propagate, then 6 for the observation); lqro_normals
 * reproduces the stream. */
#define LQRO_NORMALS_PER_AGENT 22

typedef struct lqro_agents {
  double* x;             /* n*16  Quadrotor::x: the estimate lqro_step reads     */
  double* rot;           /* n*9   Quadrotor::Rot                                 */
  double* x_true;        /* n*16  Quadrotor::xTrue                               */
  double* rot_true;      /* n*9   Quadrotor::RotTrue                             */
  double* P;             /* n*256 Quadrotor::P, state covariance                 */
  double* vgoal;         /* n*3   in: newV (lqro_step); out: findVGoal()         */
  double* u;             /* n*4   out: findU(); may be NULL                      */
  const double* u_goal;  /* n*4   Quadrotor::uGoal                               */
  const double* p_goal;  /* n*3   Quadrotor::pGoal                               */
  const double* L;       /* U*X   gains (Quadrotor::L,E,l,Lh,Eh): one block, or  */
  const double* E;       /* U*3     n blocks with per_agent_gains = 1            */
  const double* l;       /* U                                                    */
  const double* Lh;      /* 3*X                                                  */
  const double* Eh;      /* 3*3                                                  */
  const double* M;       /* X*X   motion noise variance (LQRO:1285)              */
  const double* N;       /* 6*6   observation noise variance (LQRO:1286)         */
  const double* normals; /* n*LQRO_NORMALS_PER_AGENT                             */
  float* keyframes;      /* n*8 out, may be NULL: Quadrotor::visualize's keyframe */
                         /*   (LQRO:128-133): time, (float) xTrue[0..2],          */
                         /*   (float) quatFromRot(RotTrue) (stdafx.h:24-33)       */
  double time;           /* t*dt, the keyframe time (LQRO:1444)                   */
} lqro_agents;

/* Host arrays; synchronous.  models: n_models = 1 (shared) or n. */
int lqro_dynamics_step(const lqro_model* models, int32_t n_models, int32_t n,
                       int32_t per_agent_gains, const lqro_agents* agents, int32_t device);
/* Device-resident: every pointer in *agents and `models` is a device pointer on
 * the current device; enqueued on `stream` (hipStream_t, NULL = default),
 * returns without synchronising.  d_x then feeds lqro_step_device directly. */
int lqro_dynamics_step_device(const lqro_model* models, int32_t n_models, int32_t n,
                              int32_t per_agent_gains, const lqro_agents* agents, void* stream);
/* normal() (LQRO:340-350) over random() (LQRO:334-337) on the MSVC rand()
 * stream (seed' = seed*214013 + 2531011, rand = (seed' >> 16) & 0x7fff; srand(s)
 * sets seed = s).  Writes `count` draws, advances *seed. */
int lqro_normals(uint32_t* seed, int64_t count, double* out);

const char* lqro_status_string(int status);
int lqro_version(void);

#ifdef __cplusplus
}
#endif
#endif /* LQRO_H */
