// A plain sequential restatement of MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth (reference
// src/MapPoint.cc:376-448, :468-532) on the arrays of gfs_map_points_problem, point after point the way the reference runs them: the
// descriptors of the point are collected, a real N x N table is filled, every row is copied and sorted, the element of index
// 0.5 * (N - 1) is its median, and the first row with the least median wins.  It shares no code with the product (the rule header,
// the kernel, the adaptor).  Build with -ffp-contract=off: float, every operation rounded once.
#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "gfs_abi.h"

namespace {

int DescriptorDistance(const uint8_t* a, const uint8_t* b) {  // ORBmatcher::DescriptorDistance: eight 32-bit words, bits counted in parallel
  int dist = 0;
  for (int i = 0; i < 8; i++) {
    uint32_t pa, pb;
    std::memcpy(&pa, a + 4 * i, 4);
    std::memcpy(&pb, b + 4 * i, 4);
    uint32_t v = pa ^ pb;
    v = v - ((v >> 1) & 0x55555555u);
    v = (v & 0x33333333u) + ((v >> 2) & 0x33333333u);
    dist += (int)((((v + (v >> 4)) & 0x0F0F0F0Fu) * 0x01010101u) >> 24);
  }
  return dist;
}

float Norm(const float* v) {  // the written rule: (x x + y y) + z z, then the square root
  const float xx = v[0] * v[0], yy = v[1] * v[1], zz = v[2] * v[2];
  const float s = xx + yy;
  return std::sqrt(s + zz);
}

}  // namespace

// ties[p]: how many rows of point p have the best median (0 where no descriptor was chosen)
extern "C" int mr_update(const gfs_map_points_problem* pr, gfs_map_points_result* res, int32_t* ties) {
  for (int p = 0; p < pr->n_points; p++) {
    const int begin = pr->obs_start[p], end = pr->obs_start[p + 1];
    res->best_obs[p] = -1;
    res->best_median[p] = -1;
    res->normal[3 * p] = res->normal[3 * p + 1] = res->normal[3 * p + 2] = 0.0f;
    res->min_dist[p] = res->max_dist[p] = 0.0f;
    res->status[p] = 0;
    if (ties) ties[p] = 0;
    if (begin == end) continue;  // observations.empty()
    // ---- ComputeDistinctiveDescriptors
    if (pr->mode == GFS_MAP_POINTS_FULL) {
      std::vector<const uint8_t*> vDescriptors;
      std::vector<int> vObs;
      for (int o = begin; o < end; o++) {
        if (!(pr->obs_flags[o] & GFS_MAP_POINT_OBS_IN_DESC)) continue;
        vDescriptors.push_back(pr->obs_desc + 32 * (size_t)o);
        vObs.push_back(o - begin);
      }
      if (!vDescriptors.empty()) {
        const size_t N = vDescriptors.size();
        std::vector<float> Distances(N * N);
        for (size_t i = 0; i < N; i++) {
          Distances[i * N + i] = 0;
          for (size_t j = i + 1; j < N; j++) {
            int distij = DescriptorDistance(vDescriptors[i], vDescriptors[j]);
            Distances[i * N + j] = distij;
            Distances[j * N + i] = distij;
          }
        }
        int BestMedian = INT_MAX;
        int BestIdx = 0;
        std::vector<int> medians(N);
        for (size_t i = 0; i < N; i++) {
          std::vector<int> vDists(Distances.begin() + i * N, Distances.begin() + i * N + N);
          std::sort(vDists.begin(), vDists.end());
          int median = vDists[0.5 * (N - 1)];
          medians[i] = median;
          if (median < BestMedian) {
            BestMedian = median;
            BestIdx = i;
          }
        }
        res->best_obs[p] = vObs[BestIdx];
        res->best_median[p] = BestMedian;
        res->status[p] |= GFS_MAP_POINT_DESC_SET;
        if (ties) ties[p] = (int32_t)std::count(medians.begin(), medians.end(), BestMedian);
      }
    }
    // ---- UpdateNormalAndDepth
    const float* Pos = pr->pos + 3 * (size_t)p;
    float normal[3] = {0.0f, 0.0f, 0.0f};
    int n = 0;
    for (int o = begin; o < end; o++) {
      if (!(pr->obs_flags[o] & GFS_MAP_POINT_OBS_IN_NORMAL)) continue;  // leftIndex != -1
      const float* Owi = pr->obs_Ow + 3 * (size_t)o;
      float normali[3];
      for (int c = 0; c < 3; c++) normali[c] = Pos[c] - Owi[c];
      const float len = Norm(normali);
      for (int c = 0; c < 3; c++) {
        const float unit = normali[c] / len;
        normal[c] = normal[c] + unit;
      }
      n++;
    }
    float PC[3];
    for (int c = 0; c < 3; c++) PC[c] = Pos[c] - pr->ref_Ow[3 * (size_t)p + c];
    const float dist = Norm(PC);
    const float levelScaleFactor = pr->level_scale[p];
    const float mfMaxDistance = dist * levelScaleFactor;
    const float mfMinDistance = mfMaxDistance / pr->max_scale[p];
    const float fn = (float)n;
    for (int c = 0; c < 3; c++) res->normal[3 * p + c] = normal[c] / fn;
    res->max_dist[p] = mfMaxDistance;
    res->min_dist[p] = mfMinDistance;
    res->status[p] |= GFS_MAP_POINT_NORMAL_SET;
  }
  return 0;
}

// what this file compiles in of the reference's choices: the median index of a row of N, and whether median a replaces best b
extern "C" void mr_constants(int N, int a, int b, int32_t* out) {
  std::vector<int> v(N);
  for (int i = 0; i < N; i++) v[i] = i;
  out[0] = v[0.5 * (N - 1)];
  out[1] = a < b ? 1 : 0;
}
