"""Timing of ComputeBoW and of the BoW database query (not bench.py).  The same bytes obtained in several ways, timed alternately in
blocks in one process:

  transform   a full synthetic k = 10, L = 6 vocabulary (1 111 111 nodes, about 36 MB of descriptors), 1 000 and 2 000 features a
              frame, one frame a call and eight
      device        the synchronous gfs_bow_transform call (staging, one upload, two kernels, one download)
      device_desc   gfs_bow_transform_device on descriptors already in HBM (no upload)
      host          the sequential restatement on one host thread (tests/host/bow_vocab_restatement.cpp), its tree built once
      host_rule     the rule header's host build on one host thread, its tree packed once
  query       500 and 5 000 entries of about 1 000 words, the query sharing a third of its words with a tenth of them
      device        the synchronous gfs_bow_db_query call: counts and scores of every slot
      host          the restatement: the inverted-file walk plus L1Scoring::score of the entries above minCommonWords

The comparison partner is NOT the reference: no DBoW2 or OpenCV build exists here.  Reports the median and p90 wall time of each over all
calls, the ratio host / device of the medians with the minimum and maximum of the per-block ratios (the run-to-run spread), and
checks that the paths return the same bytes.  Prints one JSON line; --out writes it.

    python tools/bench_bow_vocab.py [--blocks 6] [--calls 10] [--out profiles/bow_vocab_bench.json] [--only NAME] [--small]
    python tools/bench_bow_vocab.py --loop 30 --only transform_n2000_b1      # only device calls (for a kernel trace)
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
LEVELSUP = 4


class Hip:
    def __init__(self):
        self.lib = C.CDLL("libamdhip64.so")  # the HIP runtime the library itself uses
        self.lib.hipMalloc.argtypes = [C.POINTER(C.c_void_p), C.c_size_t]
        self.lib.hipMemcpy.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int]

    def to_device(self, a):
        p = C.c_void_p()
        assert self.lib.hipMalloc(C.byref(p), max(a.nbytes, 4)) == 0 and self.lib.hipMemcpy(p, a.ctypes.data, a.nbytes, 1) == 0
        return p


class TransformJob:
    paths = ("device", "device_desc", "host", "host_rule")

    def __init__(self, shared, n, B):
        import bow_vocab_support as BV
        from geoflowslam_amd import api, synth
        self.api, self.BV, self.n, self.B = api, BV, n, B
        self.voc, self.R, self.L = shared["voc"], BV.restatement(), api.lib()
        self.tree, self.packed = shared["tree"], shared["packed"]
        self.descs = [synth.bow_features(500 + 17 * b + n, shared["vocab"], n, 10, 0.1) for b in range(B)]
        self.ptrs = (C.c_void_p * B)(*[d.ctypes.data for d in self.descs])
        self.counts = np.full(B, n, np.int32)
        stride = shared["max_features"]
        packed = np.zeros((B, stride, 32), np.uint8)
        for b, d in enumerate(self.descs):
            packed[b, :n] = d
        self.stride, self.d_desc, self.d_counts = stride, shared["hip"].to_device(packed), shared["hip"].to_device(self.counts)
        self.out = {k: api.bow_vectors_alloc(B, stride) for k in self.paths}
        vp, i = C.c_void_p, C.c_int
        for f in (self.R.bv_vocabulary_transform, self.R.bv_rule_tree_transform):
            f.argtypes = [vp, C.POINTER(vp), vp, i, i, C.POINTER(api.BowVectors)]

    def device(self):
        assert self.L.gfs_bow_transform(self.voc.h, self.ptrs, self.counts.ctypes.data, self.B, LEVELSUP, self.out["device"][0]) == 0, self.L.gfs_last_error()

    def device_desc(self):
        assert self.L.gfs_bow_transform_device(self.voc.h, self.d_desc, self.d_counts, self.stride, self.B, LEVELSUP, self.out["device_desc"][0]) == 0, \
            self.L.gfs_last_error()

    def host(self):
        assert self.R.bv_vocabulary_transform(self.tree, self.ptrs, self.counts.ctypes.data, self.B, LEVELSUP, self.out["host"][0]) == 0

    def host_rule(self):
        assert self.R.bv_rule_tree_transform(self.packed, self.ptrs, self.counts.ctypes.data, self.B, LEVELSUP, self.out["host_rule"][0]) == 0

    def same(self):
        res = {k: self.api.bow_vectors_results(*self.out[k], self.counts) for k in self.paths}
        ok = True
        for k in self.paths[1:]:
            for a, b in zip(res["device"], res[k]):
                ok = ok and all(a[f].tobytes() == b[f].tobytes() for f in ("word_id", "word_value", "node_id", "node_start", "feat_idx"))
        return ok

    def info(self):
        r = self.api.bow_vectors_results(*self.out["device"], self.counts)
        return dict(features=self.n, batch=self.B, words=[len(x["word_id"]) for x in r], nodes=[len(x["node_id"]) for x in r])


class QueryJob:
    paths = ("device", "host")

    def __init__(self, E, n_words=1000, id_range=1000000, places=10, max_words=2048):
        import bow_vocab_support as BV
        from geoflowslam_amd import api
        self.api, self.BV, self.E = api, BV, E
        rng = np.random.default_rng(E)
        pools = [rng.choice(id_range, 3 * n_words, replace=False) for _ in range(places)]
        frequent = rng.choice(id_range, 2000, replace=False)

        def vector(place, seed):
            ids = np.unique(np.concatenate([rng.choice(pools[place], n_words - 100, replace=False), rng.choice(frequent, 100, replace=False)]))
            return BV.bow_vector(seed, 0, 0, ids=ids)
        self.dev, self.ref = api.BowDatabase(E, max_words), BV.RestatedDatabase(E)
        for s in rng.permutation(E):
            v = vector(int(s) % places, int(s))
            self.dev.add(int(s), *v)
            self.ref.add(int(s), *v)
        self.q = vector(0, 10 ** 6)
        self.L, self.R = api.lib(), BV.restatement()
        self.R.bv_db_query_above.argtypes = self.R.bv_db_query.argtypes
        self.out = {k: dict(n_common=np.zeros(E, np.int32), first_word=np.zeros(E, np.int32), score=np.zeros(E, np.float32)) for k in self.paths}
        self.list = np.zeros(E, np.int32)

    def _args(self, k):
        o = self.out[k]
        return [len(self.q[0]), self.q[0].ctypes.data, self.q[1].ctypes.data, o["n_common"].ctypes.data, o["first_word"].ctypes.data, o["score"].ctypes.data]

    def device(self):
        assert self.L.gfs_bow_db_query(self.dev.h, *self._args("device")) == 0, self.L.gfs_last_error()

    def host(self):
        self.n_list = self.R.bv_db_query_above(self.ref.h, *self._args("host"), self.list.ctypes.data)

    def same(self):
        d, h = self.out["device"], self.out["host"]
        scored = h["score"] != 0
        return bool(d["n_common"].tobytes() == h["n_common"].tobytes() and d["first_word"].tobytes() == h["first_word"].tobytes() and
                    scored.any() and d["score"][scored].tobytes() == h["score"][scored].tobytes())

    def info(self):
        d, h = self.out["device"], self.out["host"]
        return dict(entries=self.E, query_words=len(self.q[0]), sharing=int((d["n_common"] > 0).sum()), max_common=int(d["n_common"].max()),
                    scored_by_host=int((h["score"] != 0).sum()), scored_by_device=int((d["n_common"] > 0).sum()))


def _timed(fn, calls):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def measure_job(j, a):
    if a.loop:
        for _ in range(a.loop):
            j.device()
        return dict(j.info(), device_calls=a.loop)
    for _ in range(3):  # warm-up
        for k in j.paths:
            getattr(j, k)()
    same = j.same()
    ts, ratios = {k: [] for k in j.paths}, {k: [] for k in j.paths if k.startswith("host")}
    for _ in range(a.blocks):
        blk = {k: _timed(getattr(j, k), a.calls) for k in j.paths}
        for k in ts:
            ts[k] += blk[k]
        for k in ratios:
            ratios[k].append(float(np.median(blk[k]) / np.median(blk["device"])))
    same = same and j.same()
    out = dict(j.info(), calls=a.blocks * a.calls, same_results=bool(same))
    for k in j.paths:
        out[k + "_ms_median"], out[k + "_ms_p90"] = float(np.median(ts[k])), float(np.percentile(ts[k], 90))
    for k, r in ratios.items():
        out["ratio_%s_over_device" % k] = out[k + "_ms_median"] / out["device_ms_median"]
        out["ratio_%s_per_block_min" % k], out["ratio_%s_per_block_max" % k] = min(r), max(r)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--blocks", type=int, default=6)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--out", default=None)
    ap.add_argument("--only", default=None, help="the workloads whose name starts with this")
    ap.add_argument("--loop", type=int, default=0, help="only run this many device calls of each workload")
    ap.add_argument("--small", action="store_true", help="a k = 10, L = 4 vocabulary and 200 entries (a quick look, not the record)")
    a = ap.parse_args()
    import bow_vocab_support as BV
    from geoflowslam_amd import api, synth
    res = {}
    want = lambda name: not a.only or name.startswith(a.only)
    shapes = [(n, B) for n in (1000, 2000) for B in (1, 8)]
    if any(want("transform_n%d_b%d" % s) for s in shapes):
        L_ = 4 if a.small else 6
        t0 = time.perf_counter()
        vocab = synth.bow_vocabulary(1, k=10, L=L_, stop_frac=0.01)
        V, keep = api.bow_vocabulary_struct(vocab)
        R = BV.restatement()
        R.bv_vocabulary_create.restype = R.bv_rule_tree_create.restype = C.c_void_p
        R.bv_vocabulary_create.argtypes = R.bv_rule_tree_create.argtypes = [C.POINTER(api.BowVocabularyStruct)]
        shared = dict(vocab=vocab, max_features=2048, hip=Hip(), voc=api.BowVocabulary(vocab, max_batch=8, max_features=2048),
                      tree=R.bv_vocabulary_create(C.byref(V)), packed=R.bv_rule_tree_create(C.byref(V)))
        res["vocabulary"] = dict(k=10, L=L_, n_nodes=int(vocab["n_nodes"]), descriptor_bytes=int(vocab["n_nodes"]) * 32, levelsup=LEVELSUP,
                                 setup_s=time.perf_counter() - t0)
        for s in shapes:
            name = "transform_n%d_b%d" % s
            if want(name):
                res[name] = measure_job(TransformJob(shared, *s), a)
    for E in ((200,) if a.small else (500, 5000)):
        name = "query_e%d" % E
        if want(name):
            res[name] = measure_job(QueryJob(E), a)
    out = dict(metric="bow_vocab", latency="wall time of the synchronous call, alternating blocks in one process",
               partner="the sequential restatement and the rule's host build on one host thread; not the reference (no DBoW2 / OpenCV build here)",
               workloads=res)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
