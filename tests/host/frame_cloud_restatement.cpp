// Sequential restatement of the frame cloud: LaserProcessingClass::featureExtraction and the tail of the
// Frame constructor, written from the section's text -- host atan2, std::sort, std::vector, one point at a time.  The GPU path
// (csrc/frame_cloud.hip) must give these bits.  Build with -ffp-contract=off.
//
//   fcr_run(...)            runs the whole chain on one cloud and keeps every stage; returns GFS_OK / the refusal's code
//   fcr_count(stage)        points of a stage: 0 edge_raw, 1 surf_raw, 2 edge_voxel, 3 surf_voxel, 4 edge, 5 surf, 6 cloud, 7 down
//   fcr_points(stage, out)  a stage's points [count][3]
//   fcr_scans(out)          the scan table [n_scans][4]: begin, count, pad flags (1 start, 2 end), candidates in the scans in front
//   fcr_info(out)           the 13 ints of gfs_frame_cloud_info (host_scan_split = 0)
//   fcr_voxel / fcr_radius  the two filters on their own
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <map>
#include <tuple>
#include <vector>

namespace {

constexpr int kOk = 0, kInvalid = -1, kCapacity = -4, kUnsupported = -5;
constexpr long long kIntMax = 2147483647LL;

struct Pt {
  float x, y, z;
};
typedef std::vector<Pt> Cloud;

struct Sorted {
  int id;
  double value;
};

Cloud g_stage[8];
std::vector<int32_t> g_scans;
int32_t g_info[13];

double degrees(float a, float b) { return std::atan2((double)a, (double)b) * 180 / M_PI; }

// pcl::VoxelGrid, the rule of DESIGN.md section 11; an empty cloud stays empty
int voxel(const Cloud& in, float leaf, Cloud* out, int* passthrough) {
  out->clear();
  *passthrough = 0;
  const int n = (int)in.size();
  if (n == 0) return kOk;
  const float inv = 1.0f / leaf;
  float mn[3] = {in[0].x, in[0].y, in[0].z}, mx[3] = {in[0].x, in[0].y, in[0].z};
  for (const Pt& p : in) {
    const float v[3] = {p.x, p.y, p.z};
    for (int a = 0; a < 3; a++) {
      mn[a] = std::min(mn[a], v[a]);
      mx[a] = std::max(mx[a], v[a]);
    }
  }
  long long cells = 1;
  for (int a = 0; a < 3; a++) {
    const float fd = (mx[a] - mn[a]) * inv;
    if (fd < 2147483648.0f) cells *= (long long)fd + 1;
    if (!(fd < 2147483648.0f) || cells > kIntMax) {  // the leaf is too small for the data: the filter returns its input
      *passthrough = 1;
      *out = in;
      return kOk;
    }
  }
  long long lo[3], div[3];
  for (int a = 0; a < 3; a++) {
    const float fl = std::floor(mn[a] * inv), fh = std::floor(mx[a] * inv);
    if (!(std::fabs(fl) < 2147483648.0f) || !(std::fabs(fh) < 2147483648.0f)) return kUnsupported;
    lo[a] = (int)fl;
    div[a] = (long long)(int)fh - lo[a] + 1;
  }
  if (div[0] * div[1] > kIntMax || div[0] * div[1] * div[2] > kIntMax) return kUnsupported;
  std::vector<std::pair<unsigned, int>> cell((size_t)n);  // (idx, input index)
  for (int i = 0; i < n; i++) {
    const float v[3] = {in[i].x, in[i].y, in[i].z};
    unsigned ijk[3];
    for (int a = 0; a < 3; a++) ijk[a] = (unsigned)(int)(std::floor(v[a] * inv) - (float)(int)lo[a]);
    cell[i] = {ijk[0] + ijk[1] * (unsigned)div[0] + ijk[2] * (unsigned)div[0] * (unsigned)div[1], i};
  }
  std::sort(cell.begin(), cell.end());  // ascending idx, ascending input index inside a voxel
  for (int j = 0; j < n;) {
    float sx = 0.0f, sy = 0.0f, sz = 0.0f;
    int e = j;
    for (; e < n && cell[e].first == cell[j].first; e++) {
      sx = sx + in[cell[e].second].x;
      sy = sy + in[cell[e].second].y;
      sz = sz + in[cell[e].second].z;
    }
    const float c = (float)(e - j);
    out->push_back(Pt{sx / c, sy / c, sz / c});
    j = e;
  }
  return kOk;
}

// RadiusOutlierRemoval under the stated rule: keep a point iff at least min_pts OTHER points have (double)d2 <= r * r,
// d2 = (dx * dx + dy * dy) + dz * dz in float.  A plain sequential filter over a cell map (cells of edge 2 r: a neighbour lies in the
// point's cell or one next to it); the tests also hold it against the count over all pairs.
void radius(const Cloud& in, double r, int min_pts, Cloud* out) {
  out->clear();
  const double edge = 2.0 * r;
  typedef std::tuple<long long, long long, long long> Key;
  std::map<Key, std::vector<int>> cells;
  auto key = [&](const Pt& p) {
    return Key((long long)std::floor(p.x / edge), (long long)std::floor(p.y / edge), (long long)std::floor(p.z / edge));
  };
  for (int i = 0; i < (int)in.size(); i++) cells[key(in[i])].push_back(i);
  const double r2 = r * r;
  for (int i = 0; i < (int)in.size(); i++) {
    const Key k = key(in[i]);
    int others = 0;
    for (long long a = -1; a <= 1; a++)
      for (long long b = -1; b <= 1; b++)
        for (long long c = -1; c <= 1; c++) {
          auto it = cells.find(Key(std::get<0>(k) + a, std::get<1>(k) + b, std::get<2>(k) + c));
          if (it == cells.end()) continue;
          for (int j : it->second) {
            if (j == i) continue;
            const float dx = in[j].x - in[i].x, dy = in[j].y - in[i].y, dz = in[j].z - in[i].z;
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            if ((double)d2 <= r2) others++;
          }
        }
    if (others >= min_pts) out->push_back(in[i]);
  }
}

// one scan: the padded points -> edge points (pick order) and surf points (ascending sorted order)
void scan_features(const Cloud& s, Cloud* edge, Cloud* surf) {
  std::vector<Sorted> cv;
  const int size = (int)s.size();
  for (int j = 5; j < size - 5; j++) {
    const float pd = s[j].x * s[j].x + s[j].y * s[j].y + s[j].z * s[j].z;
    const float fx = s[j - 5].x + s[j - 4].x + s[j - 3].x + s[j - 2].x + s[j - 1].x - 10 * s[j].x + s[j + 1].x + s[j + 2].x + s[j + 3].x +
                     s[j + 4].x + s[j + 5].x;
    const float fy = s[j - 5].y + s[j - 4].y + s[j - 3].y + s[j - 2].y + s[j - 1].y - 10 * s[j].y + s[j + 1].y + s[j + 2].y + s[j + 3].y +
                     s[j + 4].y + s[j + 5].y;
    const float fz = s[j - 5].z + s[j - 4].z + s[j - 3].z + s[j - 2].z + s[j - 1].z - 10 * s[j].z + s[j + 1].z + s[j + 2].z + s[j + 3].z +
                     s[j + 4].z + s[j + 5].z;
    const double point_distance = pd, diffX = fx, diffY = fy, diffZ = fz;
    cv.push_back(Sorted{j, diffX * diffX + diffY * diffY + diffZ * diffZ / point_distance});
  }
  std::sort(cv.begin(), cv.end(), [](const Sorted& a, const Sorted& b) { return a.value < b.value; });
  std::vector<char> picked((size_t)size, 0), is_edge((size_t)size, 0);
  int picks = 0;
  for (int i = (int)cv.size() - 1; i >= 0; i--) {
    const int id = cv[i].id;
    if (picked[id]) continue;
    if (cv[i].value <= 0.1) break;
    picks++;
    picked[id] = 1;
    if (picks <= 10) {
      is_edge[id] = 1;
      edge->push_back(s[id]);
    } else {
      break;
    }
    for (int k = -5; k <= 5; k++) picked[id + k] = 1;
  }
  for (const Sorted& c : cv)
    if (!is_edge[c.id]) surf->push_back(s[c.id]);
}

}  // namespace

extern "C" {

int fcr_run(const float* xyzw, int n, double horizontal_angle, double max_distance, double resolution, float downsize) {
  for (Cloud& c : g_stage) c.clear();
  g_scans.clear();
  std::memset(g_info, 0, sizeof g_info);
  g_info[0] = n;
  if (n < 1) return kInvalid;
  if (!(resolution > 0.0) || !std::isfinite(resolution) || !(downsize > 0.0f) || !std::isfinite(downsize)) return kInvalid;
  for (int i = 0; i < n; i++) {
    const float* p = xyzw + 4 * i;
    for (int a = 0; a < 3; a++)
      if (!std::isfinite(p[a]) || !(std::fabs(p[a]) < 1e6f)) return kInvalid;
    if (!(p[0] * p[0] + p[1] * p[1] + p[2] * p[2] > 0.0f)) return kInvalid;  // the curvature divides by it
  }
  // the scan split: a chain of breaks; the run open at the end of the cloud is dropped
  std::vector<Cloud> scans;
  double last_angle = degrees(xyzw[1], xyzw[2]);
  int count = 0, candidates = 0;
  bool too_long = false;
  for (int i = 0; i < n; i++) {
    const double angle = degrees(xyzw[4 * i + 1], xyzw[4 * i + 2]);
    if (std::fabs(angle - last_angle) > 0.05) {
      if (count > 20) {
        Cloud s;
        const float* first = xyzw + 4 * (i - count);
        const float* last = xyzw + 4 * (i - 1);
        int pad = 0;
        if (degrees(first[0], first[2]) > -horizontal_angle / 2.0 + 5.0) {
          pad |= 1;
          for (int k = 0; k < 5; k++) s.push_back(Pt{first[0], first[1], (float)max_distance});
        }
        for (int k = 0; k < count; k++) s.push_back(Pt{first[4 * k], first[4 * k + 1], first[4 * k + 2]});
        if (degrees(last[0], last[2]) < horizontal_angle / 2.0 - 5.0) {
          pad |= 2;
          for (int k = 0; k < 5; k++) s.push_back(Pt{last[0], last[1], (float)max_distance});
        }
        const int32_t row[4] = {i - count, count, pad, candidates};
        g_scans.insert(g_scans.end(), row, row + 4);
        candidates += (int)s.size() - 10;
        if ((int)s.size() - 10 > 1024) too_long = true;
        scans.push_back(s);
      }
      count = 0;
      last_angle = angle;
    }
    count++;
  }
  if (too_long) {
    g_scans.clear();
    return kCapacity;
  }
  for (const Cloud& s : scans) scan_features(s, &g_stage[0], &g_stage[1]);
  int pass[3];
  int rc = voxel(g_stage[0], (float)(resolution / 4.0), &g_stage[2], &pass[0]);
  if (!rc) rc = voxel(g_stage[1], (float)(resolution / 2.0), &g_stage[3], &pass[1]);
  if (!rc) {
    radius(g_stage[2], resolution, 3, &g_stage[4]);
    radius(g_stage[3], resolution, 14, &g_stage[5]);
    g_stage[6] = g_stage[5];  // surf first
    g_stage[6].insert(g_stage[6].end(), g_stage[4].begin(), g_stage[4].end());
    rc = voxel(g_stage[6], downsize, &g_stage[7], &pass[2]);
  }
  if (rc) {
    for (Cloud& c : g_stage) c.clear();
    g_scans.clear();
    return rc;
  }
  const int32_t info[13] = {n,
                            (int32_t)scans.size(),
                            (int32_t)g_stage[0].size(),
                            (int32_t)g_stage[1].size(),
                            (int32_t)g_stage[2].size(),
                            (int32_t)g_stage[3].size(),
                            (int32_t)g_stage[4].size(),
                            (int32_t)g_stage[5].size(),
                            (int32_t)g_stage[7].size(),
                            0,
                            pass[0],
                            pass[1],
                            pass[2]};
  std::memcpy(g_info, info, sizeof info);
  return kOk;
}

int fcr_count(int stage) { return (int)g_stage[stage].size(); }
void fcr_points(int stage, float* out) {
  if (!g_stage[stage].empty()) std::memcpy(out, g_stage[stage].data(), g_stage[stage].size() * sizeof(Pt));
}
int fcr_scan_count() { return (int)g_scans.size() / 4; }
void fcr_scans(int32_t* out) {
  if (!g_scans.empty()) std::memcpy(out, g_scans.data(), g_scans.size() * 4);
}
void fcr_info(int32_t* out) { std::memcpy(out, g_info, sizeof g_info); }

// the filters on their own: xyz [n][3] -> out (room for n points); return the output count, or a negative refusal
int fcr_voxel(const float* xyz, int n, float leaf, float* out, int* passthrough) {
  Cloud in((size_t)n), o;
  if (n) std::memcpy(in.data(), xyz, (size_t)n * sizeof(Pt));
  const int rc = voxel(in, leaf, &o, passthrough);
  if (rc) return rc;
  if (!o.empty()) std::memcpy(out, o.data(), o.size() * sizeof(Pt));
  return (int)o.size();
}
int fcr_radius(const float* xyz, int n, double r, int min_pts, float* out) {
  Cloud in((size_t)n), o;
  if (n) std::memcpy(in.data(), xyz, (size_t)n * sizeof(Pt));
  radius(in, r, min_pts, &o);
  if (!o.empty()) std::memcpy(out, o.data(), o.size() * sizeof(Pt));
  return (int)o.size();
}

}  // extern "C"
