// Host check of the staging-block layouts (geoflowslam_amd/csrc/staging.hpp, block_layouts.hpp): every field's offset and every
// block's size against the closed-form sums the handles computed by hand before the helper existed (written out below, `up` = round
// up to the block's alignment), at sizes that are no multiple of the alignment; fields in order and not overlapping; at() aligned for
// its element type; a field of no items takes no bytes.  Plain C++: g++ -std=c++17 -I <repo root>; exit code 0 and "ok" when all hold.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "geoflowslam_amd/csrc/block_layouts.hpp"

using namespace gfs;

static int g_bad = 0, g_checked = 0;
alignas(256) static uint8_t g_base[1 << 20];  // larger than any block below; at() is compared, never dereferenced

template <size_t N>
struct alignas(4) Hdr {  // stands for a device header struct of N bytes
  unsigned char b[N];
};

// walks the fields of one block in order
struct Walk {
  const char* what;
  size_t align, end = 0;  // end of the previous field's items
  Walk(const char* w, size_t a) : what(w), align(a) {}
  template <class T, int K>
  Walk& f(const char* name, const Field<T, K>& fld, size_t items, size_t expect_off) {
    g_checked++;
    const size_t used = items * K * sizeof(T);
    const bool ok = fld.off == expect_off && fld.off >= end && fld.off % align == 0 && fld.bytes(items) == used &&
                    reinterpret_cast<uintptr_t>(fld.at(g_base)) % alignof(T) == 0 &&
                    reinterpret_cast<const uint8_t*>(fld.at(g_base)) == g_base + fld.off &&
                    reinterpret_cast<const uint8_t*>(fld.at(g_base, 2)) == g_base + fld.off + 2 * K * sizeof(T);
    if (!ok) {
      g_bad++;
      printf("BAD %s.%s: off %zu expected %zu, previous end %zu\n", what, name, fld.off, expect_off, end);
    }
    end = fld.off + used;
    return *this;
  }
  void total(size_t bytes, size_t expect) {
    g_checked++;
    if (bytes != expect || bytes < end || bytes % align) {
      g_bad++;
      printf("BAD %s: %zu bytes expected %zu, last end %zu\n", what, bytes, expect, end);
    }
  }
};

static size_t up(size_t v) { return (v + 255) / 256 * 256; }
static size_t up64(size_t v) { return (v + 63) / 64 * 64; }

int main() {
  const size_t Bs[2] = {1, 3}, Ns[5] = {0, 1, 63, 64, 65};
  {  // the cursor itself: a field of no items takes nothing, the next one starts where it did
    Block<256> b;
    const Field<int> a{b, 0}, c{b, 1};
    const Field<double, 3> d{b, 0};
    g_checked++;
    if (a.off != 0 || c.off != 0 || d.off != 256 || b.bytes() != 256) g_bad++, printf("BAD zero-count fields\n");
  }
  for (size_t B : Bs)
    for (size_t n1 : Ns)
      for (size_t n2 : Ns) {
        {  // sbp.hip: strides SL = n1, SC = n2
          using P = Hdr<200>;
          const SbpLayout<P> Y{B, (int)n1, (int)n2};
          const size_t L = n1 * B, C = n2 * B;
          const size_t o_xw = up(B * sizeof(P)), o_desc = o_xw + up(L * 12), o_oct = o_desc + up(L * 32), o_ang = o_oct + up(L * 4),
                       o_lobs = o_ang + up(L * 4), o_kp = o_lobs + up(L), o_ur = o_kp + up(C * sizeof(gfs_keypoint)), o_cdesc = o_ur + up(C * 4),
                       o_cobs = o_cdesc + up(C * 32), in_bytes = o_cobs + up(C), r_nm = up(C * 4), res_bytes = r_nm + up(B * 4);
          Walk w("sbp.in", 256);
          w.f("pairs", Y.pairs, B, 0).f("xw", Y.xw, L, o_xw).f("desc", Y.desc, L, o_desc).f("oct", Y.oct, L, o_oct).f("ang", Y.ang, L, o_ang);
          w.f("lobs", Y.lobs, L, o_lobs).f("kp", Y.kp, C, o_kp).f("ur", Y.ur, C, o_ur).f("cdesc", Y.cdesc, C, o_cdesc).f("cobs", Y.cobs, C, o_cobs);
          w.total(Y.in.bytes(), in_bytes);
          Walk r("sbp.res", 256);
          r.f("match", Y.match, C, 0).f("nm", Y.nm, B, r_nm).total(Y.res.bytes(), res_bytes);
        }
        for (size_t n3 : {n1, n2}) {  // local_points.hip: SM = n1, SL = n3, SC = n2
          using F = Hdr<112>;
          using Me = Hdr<16>;
          const LocalLayout<F, Me> Y{B, (int)n1, (int)n3, (int)n2};
          const size_t M = n1 * B;
          const size_t i_xw = up(B * sizeof(F)), i_nrm = i_xw + up(M * 12), i_min = i_nrm + up(M * 12), i_max = i_min + up(M * 4),
                       i_desc = i_max + up(M * 4), i_obs = i_desc + up(M * 32), in_bytes = i_obs + up(M);
          const size_t o_view = up(B * sizeof(Me)), o_proj = o_view + up(M), o_depth = o_proj + up(M * 12), o_cos = o_depth + up(M * 4),
                       o_level = o_cos + up(M * 4), o_index = o_level + up(M * 4), o_match = o_index + up(n3 * B * 4),
                       o_nm = o_match + up(n2 * B * 4), out_bytes = o_nm + up(B * 4);
          Walk w("local.in", 256);
          w.f("frames", Y.frames, B, 0).f("xw", Y.xw, M, i_xw).f("nrm", Y.nrm, M, i_nrm).f("dmin", Y.dmin, M, i_min).f("dmax", Y.dmax, M, i_max);
          w.f("desc", Y.desc, M, i_desc).f("obs", Y.obs, M, i_obs).total(Y.in.bytes(), in_bytes);
          Walk o("local.out", 256);
          o.f("meta", Y.meta, B, 0).f("view", Y.view, M, o_view).f("proj", Y.proj, M, o_proj).f("depth", Y.depth, M, o_depth).f("cos", Y.cos, M, o_cos);
          o.f("level", Y.level, M, o_level).f("index", Y.index, n3 * B, o_index).f("match", Y.match, n2 * B, o_match).f("nm", Y.nm, B, o_nm);
          o.total(Y.out.bytes(), out_bytes);
        }
        for (size_t O : {n2, 2 * n2 + 1}) {  // fuse.hip: T = n1 points, B key frames of SC = n2 key-points, O slots; then sim3_search.hip
          using Q = Hdr<228>;
          const FuseLayout<Q> Y{n1, B, n2, O};
          const size_t T = n1, SC = n2;
          const size_t p_nrm = up(T * 12), p_min = p_nrm + up(T * 12), p_max = p_min + up(T * 4), p_desc = p_max + up(T * 4),
                       pts_bytes = p_desc + up(T * 32);
          const size_t k_xy = up(B * sizeof(Q)), k_ur = k_xy + up(B * SC * 8), k_oct = k_ur + up(B * SC * 4), k_desc = k_oct + up(B * SC),
                       kf_bytes = k_desc + up(B * SC * 32);
          const size_t o_idx = up(O), o_dist = o_idx + up(O * 4), o_level = o_dist + up(O * 4), out_bytes = o_level + up(O * 4);
          Walk p("fuse.pts", 256);
          p.f("xw", Y.p.xw, T, 0).f("nrm", Y.p.nrm, T, p_nrm).f("dmin", Y.p.dmin, T, p_min).f("dmax", Y.p.dmax, T, p_max).f("desc", Y.p.desc, T, p_desc);
          p.total(Y.pts.bytes(), pts_bytes);
          Walk k("fuse.kf", 256);
          k.f("problems", Y.problems, B, 0).f("xy", Y.xy, B * SC, k_xy).f("ur", Y.ur, B * SC, k_ur).f("oct", Y.oct, B * SC, k_oct);
          k.f("kdesc", Y.kdesc, B * SC, k_desc).total(Y.kf.bytes(), kf_bytes);
          Walk o("fuse.out", 256);
          o.f("exit", Y.exit, O, 0).f("idx", Y.idx, O, o_idx).f("dist", Y.dist, O, o_dist).f("level", Y.level, O, o_level).total(Y.out.bytes(), out_bytes);
          // sim3_search.hip: the same point block; the key frames without mvuRight; O slots and OC = 3 O + 1 listed candidates
          const size_t OC = 3 * O + 1;
          const Sim3SearchLayout<Q> Z{n1, B, n2, O, OC};
          const size_t z_oct = k_xy + up(B * SC * 8), z_desc = z_oct + up(B * SC), z_kf_bytes = z_desc + up(B * SC * 32);
          const size_t z_level = up(O), z_count = z_level + up(O * 4), z_cidx = z_count + up(O * 4), z_cdist = z_cidx + up(OC * 4),
                       z_out_bytes = z_cdist + up(OC * 4);
          Walk zp("sim3_search.pts", 256);
          zp.f("xw", Z.p.xw, T, 0).f("nrm", Z.p.nrm, T, p_nrm).f("dmin", Z.p.dmin, T, p_min).f("dmax", Z.p.dmax, T, p_max).f("desc", Z.p.desc, T, p_desc);
          zp.total(Z.pts.bytes(), pts_bytes);
          Walk zk("sim3_search.kf", 256);
          zk.f("problems", Z.problems, B, 0).f("xy", Z.xy, B * SC, k_xy).f("oct", Z.oct, B * SC, z_oct).f("kdesc", Z.kdesc, B * SC, z_desc);
          zk.total(Z.kf.bytes(), z_kf_bytes);
          Walk zo("sim3_search.out", 256);
          zo.f("exit", Z.exit, O, 0).f("level", Z.level, O, z_level).f("count", Z.count, O, z_count).f("cidx", Z.cidx, OC, z_cidx);
          zo.f("cdist", Z.cdist, OC, z_cdist).total(Z.out.bytes(), z_out_bytes);
        }
        {  // triangulate.hip: B problems, n1 slots, n1 + B frames, n2 matrix offsets, then a key frame of n1 key-points, n2 nodes, n2 features
          using Pr = Hdr<40>;
          using Sl = Hdr<32>;
          using Fr = Hdr<276>;
          TriHeadLayout<Pr, Sl, Fr> Y{B, n1, n1 + B, n2};
          const size_t o_slot = up(B * sizeof(Pr)), o_frame = o_slot + up(n1 * sizeof(Sl)), o_pair = o_frame + up((n1 + B) * sizeof(Fr)),
                       head = o_pair + up(n2 * 4);
          Walk w("tri.in", 256);
          w.f("probs", Y.probs, B, 0).f("slots", Y.slots, n1, o_slot).f("frames", Y.frames, n1 + B, o_frame).f("pairs", Y.pairs, n2, o_pair);
          w.total(Y.in.bytes(), head);
          const size_t n = n1, m = n2, nf = n2;
          const TriKfArrays A{Y.in, n, m, nf};
          const size_t o_kps = head + up(n * 8), o_ang = o_kps + up(n * 8), o_ur = o_ang + up(n * 4), o_depth = o_ur + up(n * 4),
                       o_oct = o_depth + up(n * 4), o_hasmp = o_oct + up(n), o_desc = o_hasmp + up(n), o_nid = o_desc + up(n * 32),
                       o_nstart = o_nid + up(m * 4), o_feat = o_nstart + up((m + 1) * 4);
          w.f("un", A.un, n, head).f("kps", A.kps, n, o_kps).f("ang", A.ang, n, o_ang).f("ur", A.ur, n, o_ur).f("depth", A.depth, n, o_depth);
          w.f("oct", A.oct, n, o_oct).f("hasmp", A.hasmp, n, o_hasmp).f("desc", A.desc, n, o_desc).f("nid", A.nid, m, o_nid);
          w.f("nstart", A.nstart, m + 1, o_nstart).f("feat", A.feat, nf, o_feat);
          // the reserve's bytes of a key frame (the old frame_bytes(n, m), every key-point listed) is what one staged key frame takes
          const size_t frame_bytes = up(n * 8) * 2 + up(n * 4) * 3 + up(n) * 2 + up(n * 32) + up(m * 4) + up((m + 1) * 4) + up(n * 4);
          Block<256> one;
          TriKfArrays{one, n, m, n};
          w.total(Y.in.bytes(), head + frame_bytes - up(n * 4) + up(nf * 4));
          Walk c("tri.capacity", 256);
          c.total(one.bytes(), frame_bytes);
          const TriOutLayout Z{n1};
          const size_t q_exit = up(n1 * 4), q_stereo = q_exit + up(n1), q_x3d = q_stereo + up(n1), out_bytes = q_x3d + up(n1 * 12);
          Walk o("tri.out", 256);
          o.f("match", Z.match, n1, 0).f("exit", Z.exit, n1, q_exit).f("stereo", Z.stereo, n1, q_stereo).f("x3d", Z.x3d, n1, q_x3d);
          o.total(Z.out.bytes(), out_bytes);
        }
        if (B == 1) {  // map_points.hip (alignment 64): P = n1 points, O = n2 observations
          const size_t P = n1, O = n2;
          const MpLayout Y{P, O};
          const size_t i_dsc_start = up64((P + 1) * 4), i_pos = i_dsc_start + up64((P + 1) * 4), i_ref = i_pos + up64(P * 12),
                       i_lscale = i_ref + up64(P * 12), i_mscale = i_lscale + up64(P * 4), i_Ow = i_mscale + up64(P * 4), i_dsc_obs = i_Ow + up64(O * 12),
                       i_flags = i_dsc_obs + up64(O * 4), i_words = i_flags + up64(O), in_bytes = i_words + up64(O * 32);
          const size_t o_median = up64(P * 4), o_normal = o_median + up64(P * 4), o_min = o_normal + up64(P * 12), o_max = o_min + up64(P * 4),
                       o_status = o_max + up64(P * 4), out_bytes = o_status + up64(P);
          Walk w("mp.in", 64);
          w.f("obs_start", Y.obs_start, P + 1, 0).f("dsc_start", Y.dsc_start, P + 1, i_dsc_start).f("pos", Y.pos, P, i_pos).f("ref", Y.ref, P, i_ref);
          w.f("lscale", Y.lscale, P, i_lscale).f("mscale", Y.mscale, P, i_mscale).f("Ow", Y.Ow, O, i_Ow).f("dsc_obs", Y.dsc_obs, O, i_dsc_obs);
          w.f("flags", Y.flags, O, i_flags).f("words", Y.words, O, i_words).total(Y.in.bytes(), in_bytes);
          Walk o("mp.out", 64);
          o.f("best", Y.best, P, 0).f("median", Y.median, P, o_median).f("normal", Y.normal, P, o_normal).f("dmin", Y.dmin, P, o_min);
          o.f("dmax", Y.dmax, P, o_max).f("status", Y.status, P, o_status).total(Y.out.bytes(), out_bytes);
        }
        {  // pose.hip: stride n1
          using F = Hdr<112>;
          using Ou = Hdr<72>;
          const PoseLayout<F, Ou> L{B, n1};
          const size_t E = n1 * B;
          const size_t o_xw = up(B * sizeof(F)), o_obs = o_xw + up(E * 24), o_w = o_obs + up(E * 24), o_st = o_w + up(E * 4), in_bytes = o_st + up(E);
          const size_t r_chi = up(B * sizeof(Ou)), r_outl = r_chi + up(E * 8), res_bytes = r_outl + up(E);
          Walk w("pose.in", 256);
          w.f("frames", L.frames, B, 0).f("xw", L.xw, E, o_xw).f("obs", L.obs, E, o_obs).f("w", L.w, E, o_w).f("stereo", L.stereo, E, o_st);
          w.total(L.in.bytes(), in_bytes);
          Walk r("pose.res", 256);
          r.f("out", L.out, B, 0).f("chi2", L.chi2, E, r_chi).f("outlier", L.outlier, E, r_outl).total(L.res.bytes(), res_bytes);
        }
        {  // pose_lidar.hip: S = n1, SC = n2
          using F = Hdr<120>;
          const PoseLidarLayout<F> L{B, n1, n2};
          const size_t S = n1, SC = n2;
          const size_t o_xw = up(B * sizeof(F)), o_obs = o_xw + up(B * S * 24), o_w = o_obs + up(B * S * 24), o_st = o_w + up(B * S * 4),
                       o_cloud = o_st + up(B * S), in_bytes = o_cloud + up(B * SC * 12);
          Walk w("pose_lidar.in", 256);
          w.f("frames", L.frames, B, 0).f("xw", L.xw, B * S, o_xw).f("obs", L.obs, B * S, o_obs).f("w", L.w, B * S, o_w);
          w.f("stereo", L.stereo, B * S, o_st).f("cloud", L.cloud, B * SC, o_cloud).total(L.in.bytes(), in_bytes);
        }
        if (B == 1) {  // lidar_map.hip: K = n1 key frames, N = n2 points
          const size_t K = n1, N = n2;
          const LidarMapLayout Y{K, N};
          const size_t o_q = up((K + 1) * 4), o_t = o_q + up(K * 16), o_cloud = o_t + up(K * 12), in_bytes = o_cloud + up(N * 12);
          Walk w("lidar_map.in", 256);
          w.f("cloud_begin", Y.cloud_begin, K + 1, 0).f("q", Y.q, K, o_q).f("t", Y.t, K, o_t).f("cloud", Y.cloud, N, o_cloud).total(Y.in.bytes(), in_bytes);
        }
      }
  printf("%s: %d checks, %d bad\n", g_bad ? "FAILED" : "ok", g_checked, g_bad);
  return g_bad ? 1 : 0;
}
