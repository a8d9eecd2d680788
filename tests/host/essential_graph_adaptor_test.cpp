// Test harness for gfs_host::OptimizeEssentialGraph (geoflowslam_amd/host/gfs_adaptors.hpp): plain-struct stand-ins for the members of
// KeyFrame / MapPoint / Map that Optimizer::OptimizeEssentialGraph touches (reference src/Optimizer.cc:2042-2413) and one fixed
// scenario that walks every `continue` of the graph construction; the adaptor flattens, solves (the host restatement,
// pose_graph_restatement.cpp, compiled in) and writes back; the caller gets the flattened problem as the solver saw it and the
// stand-ins as the adaptor left them.  Built by tests/test_essential_graph_adaptor.py with g++.
//
// The scenario: eight key-frames, index k with mnId kIds[k], parent k - 1, child k + 1, on a gentle arc.
//   K2 is bad: no vertex.  K3's parent is K2: the whole of K3 is skipped (:2224-2225), its covisible K0 (150) with it.
//   K0 is the init key-frame (fixed), the loop key-frame; K7 is the current one.
//   LoopConnections: K6 -> {K0 (130)};  K7 -> {K0 (weight 0, spared as the (cur, loop) pair), K1 (120), K4 (50: dropped)}.
//   Loop edges: K4 - K0, K5 - K1, K5 - K2 (no vertex: that edge alone is skipped, :2254).
//   Covisibles by weight: K4: K5 (110, younger: no edge);  K5: K3 (110);  K6: K4 (101);  K7: K6 (300, the parent), K5 (200),
//     K1 (120, already a loop connection), K4 (50, below minFeat).
//   Inertial: K6 -> mPrevKF K5;  K4 -> mPrevKF K2 (no vertex: :2345-2347).
//   CorrectedSim3 and NonCorrectedSim3 hold K6 and K7.
//   Registrations (use_icp): (target K0, source K4) accepted, (K1, K5) refused with 50 inliers.
//   Map points: P0 ref K1; P1 bad; P2 corrected by K7 with mnCorrectedReference = K6 (its reference key-frame K1 is not used);
//     P3 ref K2 (no vertex: keeps its position); P4 ref K7; P5 corrected by another key-frame: ref K5.
#include <cstring>

#include "../../geoflowslam_amd/host/gfs_adaptors.hpp"
#include "pose_graph_restatement.cpp"

namespace {
struct MockSim3 {
  double v[8];
};
struct MockKeyFrame {
  unsigned long mnId = 0;
  bool bad = false, bImu = false;
  MockKeyFrame* parent = nullptr;
  MockKeyFrame* mPrevKF = nullptr;
  std::set<MockKeyFrame*> loop_edges, children;
  std::vector<std::pair<MockKeyFrame*, int>> covisibles;  // in the order GetCovisiblesByWeight returns them
  double q[4] = {0, 0, 0, 1}, t[3] = {0, 0, 0};
  float out_q[4] = {0, 0, 0, 0}, out_t[3] = {0, 0, 0};
  int n_set_pose = 0;
  bool isBad() const { return bad; }
  MockKeyFrame* GetParent() const { return parent; }
  std::set<MockKeyFrame*> GetLoopEdges() const { return loop_edges; }
  bool hasChild(MockKeyFrame* k) const { return children.count(k) != 0; }
  int GetWeight(MockKeyFrame* k) const {
    for (const auto& c : covisibles)
      if (c.first == k) return c.second;
    return 0;
  }
  std::vector<MockKeyFrame*> GetCovisiblesByWeight(int w) const {
    std::vector<MockKeyFrame*> out;
    for (const auto& c : covisibles)
      if (c.second >= w) out.push_back(c.first);
    return out;
  }
};
struct MockMapPoint {
  bool bad = false;
  float pos[3] = {0, 0, 0};
  unsigned long mnCorrectedByKF = 0, mnCorrectedReference = 0;
  MockKeyFrame* ref = nullptr;
  int n_set_pos = 0, n_update = 0;
  bool isBad() const { return bad; }
  MockKeyFrame* GetReferenceKeyFrame() const { return ref; }
  void UpdateNormalAndDepth() { n_update++; }
};
struct MockMap {
  unsigned long init_id = ~0ul;
  std::vector<MockKeyFrame*> kfs;
  std::vector<MockMapPoint*> mps;
  std::mutex mMutexMapUpdate;
  int change_index = 0;
  unsigned long GetInitKFid() const { return init_id; }
  std::vector<MockKeyFrame*> GetAllKeyFrames() const { return kfs; }
  std::vector<MockMapPoint*> GetAllMapPoints() const { return mps; }
  void IncreaseChangeIndex() { change_index++; }
};
struct MockAccess {
  static void pose_d(const MockKeyFrame* k, double q[4], double t[3]) {
    std::memcpy(q, k->q, 32);
    std::memcpy(t, k->t, 24);
  }
  static void sim3(const MockSim3& s, double S[8]) { std::memcpy(S, s.v, 64); }
  static void set_pose(MockKeyFrame* k, const float q[4], const float t[3]) {
    std::memcpy(k->out_q, q, 16);
    std::memcpy(k->out_t, t, 12);
    k->n_set_pose++;
  }
  static void world_pos(const MockMapPoint* p, float x[3]) { std::memcpy(x, p->pos, 12); }
  static void set_world_pos(MockMapPoint* p, const float x[3]) {
    std::memcpy(p->pos, x, 12);
    p->n_set_pos++;
  }
};
constexpr int kKF = 8, kMP = 6;
const unsigned long kIds[kKF] = {3, 5, 6, 8, 9, 11, 12, 14};
}  // namespace

// kf_sim3 [8][8]: every key-frame's pose as a Sim3 of scale 1 (NonCorrectedSim3 for K6, K7); corrected [2][8]: CorrectedSim3 of K6, K7.
// flat_n = {vertices, edges, points}; the flattened arrays have room for 8 vertices, 32 edges, 6 points.  reg_calls [.][2 + 16]: target
// id, source id and the init matrix of every registration.  kf_out [8][8]: SetPose's q, t and the call count; mp_out [6][5]: position,
// SetWorldPos calls, UpdateNormalAndDepth calls.  counts = {solves, fix_scale, iterations, registrations, change index} and
// lambda_init.  Returns 0, or -1 on an exception.
extern "C" int essential_graph_adaptor_test(int fix_scale, int use_icp, double* kf_sim3, double* corrected, int32_t* flat_n, double* vq,
                                            double* vt, double* vs, uint8_t* vfixed, int32_t* ei, int32_t* ej, double* eq, double* et,
                                            double* es, double* ew, float* points, int32_t* pref, double* sol_q, double* sol_t,
                                            double* sol_s, float* sol_points, double* reg_calls, float* kf_out, float* mp_out,
                                            int32_t* counts, double* lambda_init) {
  try {
    MockMap map;
    std::vector<MockKeyFrame> K(kKF);
    std::vector<MockMapPoint> P(kMP);
    for (int k = 0; k < kKF; k++) {
      K[k].mnId = kIds[k];
      const double a = 0.1 * k;
      K[k].q[2] = std::sin(a / 2);
      K[k].q[3] = std::cos(a / 2);
      K[k].t[0] = 0.5 * k;
      K[k].t[1] = 0.1 * k * k;
      K[k].t[2] = 0.02 * k;
      if (k > 0) K[k].parent = &K[k - 1];
      if (k + 1 < kKF) K[k].children.insert(&K[k + 1]);
      map.kfs.push_back(&K[k]);
      std::memcpy(kf_sim3 + 8 * k, K[k].q, 32);
      std::memcpy(kf_sim3 + 8 * k + 4, K[k].t, 24);
      kf_sim3[8 * k + 7] = 1.0;
    }
    K[2].bad = true;
    map.init_id = K[0].mnId;
    auto link = [&](int a, int b) {
      K[a].loop_edges.insert(&K[b]);
      K[b].loop_edges.insert(&K[a]);
    };
    link(4, 0);
    link(5, 1);
    link(5, 2);
    K[3].covisibles = {{&K[0], 150}};
    K[4].covisibles = {{&K[5], 110}};
    K[5].covisibles = {{&K[3], 110}};
    K[6].covisibles = {{&K[0], 130}, {&K[4], 101}};
    K[7].covisibles = {{&K[6], 300}, {&K[5], 200}, {&K[1], 120}, {&K[4], 50}};
    K[6].bImu = true;
    K[6].mPrevKF = &K[5];
    K[4].bImu = true;
    K[4].mPrevKF = &K[2];
    std::map<MockKeyFrame*, std::set<MockKeyFrame*>> LoopConnections;
    LoopConnections[&K[6]] = {&K[0]};
    LoopConnections[&K[7]] = {&K[0], &K[1], &K[4]};
    std::map<MockKeyFrame*, MockSim3> Corrected, NonCorrected;
    for (int c = 0; c < 2; c++) {
      const int k = 6 + c;
      MockSim3 nc, co;
      std::memcpy(nc.v, kf_sim3 + 8 * k, 64);
      const double s = fix_scale ? 1.0 : 1.1, a = 0.1 * k - 0.03;
      const double v[8] = {0.01, -0.005, std::sin(a / 2), std::cos(a / 2), s * (0.5 * k - 0.2), s * (0.1 * k * k + 0.15), s * 0.02 * k, s};
      std::memcpy(co.v, v, 64);
      std::memcpy(corrected + 8 * c, v, 64);
      NonCorrected[&K[k]] = nc;
      Corrected[&K[k]] = co;
    }
    for (int m = 0; m < kMP; m++) {
      P[m].pos[0] = 1.f + 0.25f * m;
      P[m].pos[1] = -0.5f + 0.125f * m;
      P[m].pos[2] = 2.f + 0.5f * m;
      map.mps.push_back(&P[m]);
    }
    P[0].ref = &K[1];
    P[1].ref = &K[1];
    P[1].bad = true;
    P[2].ref = &K[1];
    P[2].mnCorrectedByKF = K[7].mnId;
    P[2].mnCorrectedReference = K[6].mnId;
    P[3].ref = &K[2];
    P[4].ref = &K[7];
    P[5].ref = &K[5];
    P[5].mnCorrectedByKF = K[4].mnId;
    P[5].mnCorrectedReference = K[0].mnId;

    int n_solves = 0, n_reg = 0;
    auto solve = [&](const gfs_essential_graph_problem& p, gfs_essential_graph_solution& s) {
      n_solves++;
      flat_n[0] = p.n_vertices;
      flat_n[1] = p.n_edges;
      flat_n[2] = p.n_points;
      if (p.n_vertices > kKF || p.n_edges > 32 || p.n_points > kMP) throw std::runtime_error("the flattened graph is larger than the scenario");
      std::memcpy(vq, p.vertex_q, 32 * p.n_vertices);
      std::memcpy(vt, p.vertex_t, 24 * p.n_vertices);
      std::memcpy(vs, p.vertex_s, 8 * p.n_vertices);
      std::memcpy(vfixed, p.vertex_fixed, p.n_vertices);
      std::memcpy(ei, p.edge_i, 4 * p.n_edges);
      std::memcpy(ej, p.edge_j, 4 * p.n_edges);
      std::memcpy(eq, p.edge_q, 32 * p.n_edges);
      std::memcpy(et, p.edge_t, 24 * p.n_edges);
      std::memcpy(es, p.edge_s, 8 * p.n_edges);
      std::memcpy(ew, p.edge_w, 8 * p.n_edges);
      std::memcpy(points, p.points, 12 * p.n_points);
      std::memcpy(pref, p.point_ref, 4 * p.n_points);
      counts[1] = p.fix_scale;
      counts[2] = p.iterations;
      *lambda_init = p.lambda_init;
      pgr_optimize(&p, &s);
      std::memcpy(sol_q, s.vertex_q, 32 * p.n_vertices);
      std::memcpy(sol_t, s.vertex_t, 24 * p.n_vertices);
      std::memcpy(sol_s, s.vertex_s, 8 * p.n_vertices);
      std::memcpy(sol_points, s.points, 12 * p.n_points);
    };
    auto reg = [&](const MockKeyFrame* target, const MockKeyFrame* source, const double init_T[16]) {
      gfs_gicp_result r{};
      reg_calls[18 * n_reg] = (double)target->mnId;
      reg_calls[18 * n_reg + 1] = (double)source->mnId;
      std::memcpy(reg_calls + 18 * n_reg + 2, init_T, 128);
      std::memcpy(r.T_target_source, init_T, 128);
      r.T_target_source[12] += 0.01;  // the registration moves the translation a little
      r.T_target_source[13] -= 0.02;
      r.converged = 1;
      r.num_inliers = n_reg == 0 ? 500 : 50;
      r.error = 1.0;
      n_reg++;
      return r;
    };
    const bool bFixScale = fix_scale != 0, bUseICP = use_icp != 0;
    gfs_host::OptimizeEssentialGraph<MockAccess>(solve, reg, &map, &K[0], &K[7], NonCorrected, Corrected, LoopConnections, bFixScale, bUseICP);
    for (int k = 0; k < kKF; k++) {
      std::memcpy(kf_out + 8 * k, K[k].out_q, 16);
      std::memcpy(kf_out + 8 * k + 4, K[k].out_t, 12);
      kf_out[8 * k + 7] = (float)K[k].n_set_pose;
    }
    for (int m = 0; m < kMP; m++) {
      std::memcpy(mp_out + 5 * m, P[m].pos, 12);
      mp_out[5 * m + 3] = (float)P[m].n_set_pos;
      mp_out[5 * m + 4] = (float)P[m].n_update;
    }
    counts[0] = n_solves;
    counts[3] = n_reg;
    counts[4] = map.change_index;
    return 0;
  } catch (const std::exception& ex) {
    fprintf(stderr, "essential_graph_adaptor_test: %s\n", ex.what());
    return -1;
  }
}
