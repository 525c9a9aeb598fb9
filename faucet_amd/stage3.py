"""A consumer of the batched Stage-3 probes: JunctionMap::findNeighbor for MANY junctions in lock-step.

The reference's contig-graph stage (out of scope of this repository) walks the Bloom filter from every junction along every
extension a contig is built on: `findNeighbor` (utils/JunctionMap.cpp:231-412) asks `getValidJExtension` (:474-490) for the one
valid next base, advances, looks the k-mer up in the junction map, and repeats until it reaches a junction or a sink.  Each call is a
chain of dependent filter probes; different calls are independent.  Here all walks advance together: ONE call of
`fgpu_probe_valid_extension` per step answers `getValidJExtension` for every walk that is still under way (the device does the
4 x (contains + jcheck) probes of each), the host does what the reference does between two probes -- advance the DoubleKmer, look
the junction map up, keep the distance and contig-length bookkeeping.  No filter bit is tested on the host.

Restated from the reference's control flow (not its text), its asserts included: a call in which the reference would trip one (:318,
:338-339, and :355 / :370 -- a junction met before maxDist must itself have exactly one valid extension) comes back with abort = 1.
Checked against the reference's own findNeighbor on the golden maps, on fresh runs at even and small k and on seeded variants of both
with thinned maps, damaged filters and shifted distances (oracle/_ref/ref_kat neighbors -> tests/golden/stage3_neighbors_*.jsonl.gz,
tests/stage3_variants.py, tests/test_stage3_walker.py).

`NeighborWalker.contigs` chains such calls into JunctionMap::getContig (:133-221) for many starts, one round of findNeighbor calls per chain
segment, with the bookkeeping on the host: what a caller had to do before fgpu_stage3_contigs (api.Context.stage3_contigs) did the whole
chain on the device.  It stays as the second implementation and as the baseline scripts/stage3_contig_times.py times.  `branching_starts`
and `linear_starts` list the getContig calls of the reference's two graph-build loops on a map that does not change.

`build_serial` is JunctionMap::buildContigGraph's loop (:11-129) itself, one getContig at a time through Context.stage3_contigs with the map set
again after every call that kills: the second implementation of fgpu_stage3_build (api.Context.stage3_build) and the baseline
scripts/stage3_build_times.py times.
"""
from __future__ import annotations

import numpy as np

NT = "ACTG"                                     # the reference's 2-bit code: A 0, C 1, T 2, G 3


def _kmer_string(x: int, k: int) -> str:
    return "".join(NT[(x >> (2 * i)) & 3] for i in range(k - 1, -1, -1))


def branching_starts(keys, recs, k: int):
    """(k-mers, indices) of the getContig calls buildBranchingPaths (utils/JunctionMap.cpp:36-50) makes on a map that does not change: every
    covered index 0..4 of every junction with more than one path out, in map order -- the first base's extension of a homopolymer k-mer
    left out (:43-47; coverage 4 is the sum of what is left)."""
    cov = np.array(recs["cov"], dtype=np.int64)
    keys = np.asarray(keys, dtype=np.uint64)
    complex_ = (cov > 0).sum(axis=1) > 1
    for r in np.nonzero(complex_)[0]:
        s = _kmer_string(int(keys[r]), k)
        if len(set(s)) == 1:
            cov[r, NT.index(s[0])] = 0
    c5 = np.concatenate([cov, cov.sum(axis=1, keepdims=True)], axis=1)
    rows, idx = np.nonzero((c5 > 0) & complex_[:, None])
    return keys[rows], idx.astype(np.int8)


def linear_starts(keys, recs):
    """(k-mers, indices) of the getContig calls buildLinearRegions (:105-118) makes: the covered extension, then 4, of every junction with
    exactly one path out, in map order"""
    cov = np.asarray(recs["cov"], dtype=np.int64)
    keys = np.asarray(keys, dtype=np.uint64)
    rows = np.nonzero((cov > 0).sum(axis=1) == 1)[0]
    idx = np.stack([(cov[rows] > 0).argmax(axis=1), np.full(len(rows), 4)], axis=1)
    return np.repeat(keys[rows], 2), idx.reshape(-1).astype(np.int8)


def build_serial(ctx, keys, recs, k: int, max_read_length: int, limit=None):
    """buildContigGraph's contig list, literally: buildBranchingPaths (:34-82), destroyComplexJunctions (:90-102), buildLinearRegions
    (:104-129), every getContig one device call on the map as it stands -- ctx.stage3_set_junctions again, without the junctions that
    are gone, after every call that kills.  Returns (calls, status, sets): one dict per call made (phase 0 branching / 1 linear forward /
    2 linear backward, start, ind1, ind2, end_kmer, end_node, string, distances, coverages, kills, far_kmer, far_is_junction, far_is_start);
    status 0, or 1 / 3 where the reference would not return from the next call; the number of times the map was set.
    limit: stop (status None) after that many calls."""
    keys = np.ascontiguousarray(keys, dtype=np.uint64)
    recs = np.ascontiguousarray(recs)
    cov = np.array(recs["cov"], dtype=np.int64)
    paths = (cov > 0).sum(axis=1)
    row_of = {int(x): r for r, x in enumerate(keys)}
    alive = np.ones(len(keys), dtype=bool)
    claimed, calls, state = set(), [], dict(stale=True, sets=0)
    code = {c: i for i, c in enumerate(NT)}

    def get_contig(r, i, own, phase):
        if state["stale"]:
            ctx.stage3_set_junctions(keys[alive], recs[alive])
            state.update(stale=False, sets=state["sets"] + 1)
        out, strings, dists, covs, kills, _ = ctx.stage3_contigs(keys[r:r + 1], [i], max_read_length)
        if int(out["status"][0]):
            return int(out["status"][0])
        c = dict(phase=phase, start=int(keys[r]), ind1=int(out["ind1"][0]), ind2=int(out["ind2"][0]), end_kmer=int(out["end_kmer"][0]),
                 end_node=int(out["end_node"][0]), string=strings[0], distances=dists[0].tolist(), coverages=covs[0].tolist(), kills=[int(x) for x in kills[0]])
        c["coverages"][0] = int(own[i] if i < 4 else own.sum()) & 0xFF                    # :148 reads the caller's copy of the junction (:43-47)
        for x in c["kills"]:                                                               # :210-216
            if x != c["start"]:
                alive[row_of[x]] = False
                state["stale"] = True
        far = 0                                                                            # Contig::getSideKmer(2), src/Contig.cpp:235-239: the last
        for ch in (c["string"][-k:] if c["ind2"] == 4 else reversed(c["string"][-k:])):   # k-mer, reverse-complemented unless ind2 is 4
            far = (far << 2) | (code[ch] if c["ind2"] == 4 else code[ch] ^ 2)
        is_j = far in row_of and bool(alive[row_of[far]])                                  # :56
        c.update(far_kmer=far, far_is_junction=int(is_j), far_is_start=int(is_j and far == c["start"]))
        calls.append(c)
        return 0

    for r in np.nonzero(paths > 1)[0]:
        own = cov[r].copy()
        s = _kmer_string(int(keys[r]), k)
        if len(set(s)) == 1:
            own[NT.index(s[0])] = 0
        for i in range(5):
            if (own[i] if i < 4 else own.sum()) > 0 and (r, i) not in claimed:             # :50
                if limit is not None and len(calls) >= limit:
                    return calls, None, state["sets"]
                status = get_contig(r, i, own, 0)
                if status:
                    return calls, status, state["sets"]
                c = calls[-1]
                claimed.add((r, c["ind1"]))                                                # setEnds, src/Contig.cpp:123-133
                if c["far_is_junction"]:
                    claimed.add((row_of[c["far_kmer"]], c["ind2"]))
    if (paths > 1).any():
        alive[paths > 1] = False
        state["stale"] = True
    for r in np.nonzero(paths == 1)[0]:
        if not alive[r]:
            continue
        for phase, i in ((1, int(np.nonzero(cov[r] > 0)[0][-1])), (2, 4)):                 # :111-118
            if limit is not None and len(calls) >= limit:
                return calls, None, state["sets"]
            status = get_contig(r, i, cov[r], phase)
            if status:
                return calls, status, state["sets"]
    return calls, 0, state["sets"]


class NeighborWalker:
    def __init__(self, ctx, keys, recs, k: int, max_read_length: int):
        """keys / recs: the junction map (oriented k-mers; records with 'dist'), e.g. from Context.junctions() or a parsed .junctions"""
        self.ctx, self.k, self.mrl = ctx, k, max_read_length
        order = np.argsort(np.asarray(keys, dtype=np.uint64), kind="stable")
        self.keys = np.asarray(keys, dtype=np.uint64)[order]
        self.dist = np.asarray(recs["dist"], dtype=np.int64)[order]
        try:
            self.cov = np.asarray(recs["cov"], dtype=np.int64)[order]           # (only contigs() reads the coverages)
        except (KeyError, ValueError):
            self.cov = None
        self.mask = np.uint64((1 << (2 * k)) - 1)
        self.steps = 0          # device calls made by the last find_neighbors
        self.probes = 0         # k-mers handed to getValidJExtension in them
        self.rounds = 0         # rounds of findNeighbor calls made by the last contigs
        self.order = order      # sorted position -> row in the caller's arrays
        self.met = None         # after find_neighbors(alive=...): per walk, the rows of the junctions its look-ups hit, visible or not
        self._alive = self._hits = None

    # ---- the reference's k-mer helpers on arrays (utils/Kmer.cpp:238-252,410-425; utils/DoubleKmer.cpp) ----
    def _revcomp(self, x):
        r = np.zeros_like(x)
        y = x.copy()
        for _ in range(self.k):
            r = (r << np.uint64(2)) | ((y & np.uint64(3)) ^ np.uint64(2))
            y >>= np.uint64(2)
        return r

    def _forward(self, km, rc, nuc):
        nuc = nuc.astype(np.uint64)
        return ((km << np.uint64(2)) | nuc) & self.mask, (rc >> np.uint64(2)) | ((nuc ^ np.uint64(2)) << np.uint64(2 * self.k - 2))

    def _is_junction(self, km, who=None):
        i = np.searchsorted(self.keys, km)
        i = np.minimum(i, len(self.keys) - 1)
        hit = self.keys[i] == km
        if self._alive is not None:                     # a junction that is gone is not found; the walk that asked still depends on it
            if who is not None:
                self._hits.append((np.asarray(who)[hit], i[hit]))
            hit = hit & self._alive[i]
        return hit, i

    def find_neighbors(self, start_kmers, indices, contigs: bool = False, alive=None):
        """(see _find_neighbors)  alive: a mask over the map's junctions, in the order of the keys handed to the constructor -- the walks see
        only the junctions it marks, as findNeighbor does on a map from which the others were erased (killJunction); afterwards `met` lists,
        per walk, the rows of every junction of the whole map that one of its look-ups hit: the answer stands for every mask that agrees
        with this one on them.  Default: the whole map, unchanged."""
        if alive is None:
            self.met = None
            return self._find_neighbors(start_kmers, indices, contigs)
        self._alive, self._hits = np.asarray(alive, dtype=bool)[self.order], []
        try:
            out = self._find_neighbors(start_kmers, indices, contigs)
            met = [[] for _ in range(len(start_kmers))]
            for who, rows in self._hits:
                for w, r in zip(who.tolist(), self.order[rows].tolist()):
                    met[w].append(r)
            self.met = [sorted(set(m)) for m in met]
        finally:
            self._alive = self._hits = None
        return out

    def _find_neighbors(self, start_kmers, indices, contigs: bool = False):
        """findNeighbor(junctionMap[start], start, index) for every pair; returns a structured array (kmer, node, rindex, dist, len,
        abort) in input order.  `abort` marks the calls in which the reference trips one of its asserts: dist <= maxDist after the first
        k-mers, a valid extension at every step up to maxDist, and a valid extension at a junction met before maxDist.
        contigs=True: (that array, the list of BfSearchResult::contig strings)."""
        k = self.k
        n = len(start_kmers)
        km = np.asarray(start_kmers, dtype=np.uint64).copy()
        idx = np.asarray(indices, dtype=np.int64)
        rc = self._revcomp(km)
        everyone = np.arange(n)
        found, where = self._is_junction(km, everyone)
        assert found.all(), "every start k-mer must be a junction of the map"
        maxd = self.dist[where, idx]
        out = np.zeros(n, dtype=[("kmer", np.uint64), ("node", np.int8), ("rindex", np.int8), ("dist", np.int32), ("len", np.int32), ("abort", np.int8)])
        done = np.zeros(n, dtype=bool)
        dist = np.ones(n, dtype=np.int64)
        ln = np.zeros(n, dtype=np.int64)
        lastnuc = np.zeros(n, dtype=np.int64)
        retidx = np.full(n, 4, dtype=np.int64)
        phase = np.zeros(n, dtype=np.int8)                      # 0: up to maxDist, 1: past it (overlapping sinks), 2: finished
        sink = np.zeros(n, dtype=out.dtype)

        def finish(m, kmer, node, rindex, d, length):
            out["kmer"][m], out["node"][m], out["rindex"][m], out["dist"][m], out["len"][m] = kmer, node, rindex, d, length
            done[m] = True
            phase[m] = 2

        def early_junction(w, rindex):
            """a junction before maxDist (:354-357, :368-372) "should be a spacer": the reference asserts that it has exactly one valid
            extension before it returns it -- one more probe of the walks in `w`, which end here either way"""
            if len(w) == 0:
                return
            ext = self.ctx.probe_valid_extension(km[w]).astype(np.int64)
            self.steps += 1
            self.probes += len(w)
            ok, bad = w[ext >= 0], w[ext < 0]
            finish(ok, km[ok], 1, rindex[ext >= 0], dist[ok], ln[ok])
            out["abort"][bad] = 1                                                # assert(getValidJExtension(doubleKmer) >= 0)
            done[bad] = True
            phase[bad] = 2

        # ---- the first one or two k-mers (:251-302)
        back = idx == 4
        km[back], rc[back] = rc[back].copy(), km[back].copy()                    # doubleKmer.reverse()
        ln[back] = k
        isj, _ = self._is_junction(km, everyone)
        m = back & isj
        finish(m, km[m], 1, 4, 1, ln[m])
        fw = ~back
        lastnuc[fw] = (rc[fw] & np.uint64(3)).astype(np.int64)
        nk, nr = self._forward(km[fw], rc[fw], idx[fw])
        km[fw], rc[fw] = nk, nr
        ln[fw] = 1 + k
        isj, _ = self._is_junction(rc, everyone)
        m = fw & isj
        finish(m, rc[m], 1, lastnuc[m], 1, ln[m])
        m = fw & ~done & (maxd == 1)
        finish(m, rc[m], 0, lastnuc[m], 1, ln[m])
        m = fw & ~done
        dist[m] = 2
        isj, _ = self._is_junction(km, everyone)
        m2 = m & isj
        finish(m2, km[m2], 1, 4, 2, ln[m2])
        text = None
        if contigs:                                                              # :254-256, :272-276: the reversed k-mer, or the first base and the k-mer behind it
            first = np.asarray(start_kmers, dtype=np.uint64) >> np.uint64(2 * k - 2)
            text = [([] if b else [int(f)]) + [(int(x) >> (2 * i)) & 3 for i in range(k - 1, -1, -1)] for b, f, x in zip(back, first, km)]
        m = ~done & (dist > maxd)                                                # the reference's assert(dist <= maxDist)
        out["abort"][m] = 1
        done[m] = True
        phase[m] = 2

        self.steps = self.probes = 0
        while True:
            # ---- leaving the first loop (:343-366): a junction exactly where expected, else this is (probably) a sink
            m = (phase == 0) & (dist >= maxd)
            if m.any():
                isj, _ = self._is_junction(km, everyone)
                j = m & isj
                finish(j, km[j], 1, retidx[j], dist[j], ln[j])
                s = m & ~isj
                sink["kmer"][s], sink["node"][s], sink["rindex"][s], sink["dist"][s], sink["len"][s] = km[s], 0, 4, dist[s], ln[s]
                phase[s] = 1
            m = (phase == 1) & (dist >= maxd + 2 * self.mrl)                     # :376, ran past every possible overlap
            out[m] = sink[m]
            phase[m] = 2
            act = np.nonzero(phase < 2)[0]
            if len(act) == 0:
                break
            # ---- ONE device call: getValidJExtension of every walk under way
            ext = self.ctx.probe_valid_extension(km[act]).astype(np.int64)
            self.steps += 1
            self.probes += len(act)
            bad = ext < 0
            a0 = act[bad & (phase[act] == 0)]                                    # assert(validExtension != -1 / -2)
            out["abort"][a0] = 1
            phase[a0] = 2
            b1 = act[bad & (phase[act] == 1)]                                    # off the real sequence: the sink stands
            out[b1] = sink[b1]
            phase[b1] = 2
            act, ext = act[~bad], ext[~bad]
            lastnuc[act] = (rc[act] & np.uint64(3)).astype(np.int64)
            nk, nr = self._forward(km[act], rc[act], ext)
            km[act], rc[act] = nk, nr
            ln[act] += 1
            if contigs:
                for w, e in zip(act, ext):
                    text[w].append(int(e))
            # backward-facing half-step
            dist[act] += 1
            km[act], rc[act] = rc[act].copy(), km[act].copy()
            retidx[act] = lastnuc[act]
            isj, wj = self._is_junction(km[act], act)
            a = phase[act] == 0
            stop = a & (dist[act] == maxd[act])                                  # break: handled at the top of the next round
            hit = a & ~stop & isj
            early_junction(act[hit], retidx[act[hit]])
            hb = ~a & isj                                                        # past maxDist: overlap test (:391-404)
            if hb.any():
                w = act[hb]
                overlap = self.dist[wj[hb], lastnuc[w]] + maxd[w] - dist[w]
                ok = overlap >= 0
                finish(w[ok], km[w[ok]], 1, lastnuc[w[ok]], dist[w[ok]], ln[w[ok]])
                out[w[~ok]] = sink[w[~ok]]
                phase[w[~ok]] = 2
            go = (phase[act] < 2) & ~stop
            act = act[go]
            # forward-facing half-step
            dist[act] += 1
            km[act], rc[act] = rc[act].copy(), km[act].copy()
            retidx[act] = 4
            isj, wj = self._is_junction(km[act], act)
            a = phase[act] == 0
            stop = a & (dist[act] == maxd[act])
            hit = a & ~stop & isj
            early_junction(act[hit], np.full(int(hit.sum()), 4, dtype=np.int64))
            hb = ~a & isj
            if hb.any():
                w = act[hb]
                overlap = self.dist[wj[hb], 4] + maxd[w] - dist[w]
                ok = overlap >= 0
                finish(w[ok], km[w[ok]], 1, 4, dist[w[ok]], ln[w[ok]])
                out[w[~ok]] = sink[w[~ok]]
                phase[w[~ok]] = 2
        if contigs:
            return out, ["".join(NT[c] for c in t[:int(ln_)]) for t, ln_ in zip(text, out["len"])]
        return out

    def contigs(self, start_kmers, indices, find=None):
        """getContig(junctionMap[start], start, index) (utils/JunctionMap.cpp:133-221) for every pair, all chains in lock-step: one `find`
        call per round answers the next findNeighbor of every chain under way.  find(kmers, indices) -> (results, contig strings);
        default: this walker's find_neighbors.  Returns a list of dicts in input order: status (0 the reference returns, 1 it trips an
        assert, 2 no such junction or index, 3 it never returns: the chain came back to a (junction, index) that is not its start),
        ind1, ind2, end_kmer, end_node, string, distances, coverages, kills -- the last five empty unless status is 0."""
        k = self.k
        find = find or (lambda km, ix: self.find_neighbors(km, ix, contigs=True))
        start_kmers = np.asarray(start_kmers, dtype=np.uint64)
        indices = np.asarray(indices, dtype=np.int64)
        cov5 = np.concatenate([self.cov, self.cov.sum(axis=1, keepdims=True)], axis=1)

        def row_of(x):
            i = min(int(np.searchsorted(self.keys, np.uint64(x))), len(self.keys) - 1)
            return i if len(self.keys) and int(self.keys[i]) == int(x) else -1

        chains, act = [], []
        for i, (x, ix) in enumerate(zip(start_kmers, indices)):
            x, ix = int(x), int(ix)
            r = row_of(x) if 0 <= ix <= 4 else -1
            c = dict(status=0 if r >= 0 else 2, ind1=0, ind2=0, end_kmer=0, end_node=0, string="", distances=[], coverages=[], kills=[])
            if r >= 0:
                c.update(ind1=ix, coverages=[int(cov5[r, ix]) & 0xFF], at=(x, ix), seen=set(),
                         string=_kmer_string(int(self._revcomp(np.array([x], dtype=np.uint64))[0]) if ix == 4 else x, k))    # :148-151
                act.append(i)
            chains.append(c)
        self.rounds = 0
        while act:
            res, strings = find(np.array([chains[i]["at"][0] for i in act], dtype=np.uint64), np.array([chains[i]["at"][1] for i in act], dtype=np.int8))
            self.rounds += 1
            nxt = []
            for i, r, text in zip(act, res, strings):
                c = chains[i]
                if r["abort"]:
                    c["status"] = 1
                    continue
                if int(r["len"]) > k:                                             # :160-162
                    c["string"] += text[k:]
                c["distances"].append(int(r["dist"]) & 0xFF)                      # :163
                c["end_kmer"], c["end_node"], c["ind2"] = int(r["kmer"]), int(r["node"]), int(r["rindex"]) if r["node"] else 4
                if not r["node"]:
                    continue
                row = row_of(int(r["kmer"]))
                c["coverages"].append(int(cov5[row, int(r["rindex"])]) & 0xFF)    # :169
                if (self.cov[row] > 0).sum() != 1 or int(r["kmer"]) == int(start_kmers[i]):   # :171-191
                    continue
                c["kills"].append(int(r["kmer"]))
                c["at"] = (int(r["kmer"]), 4 if r["rindex"] < 4 else int((self.cov[row] > 0).argmax()))   # getOppositeIndex
                if c["at"] in c["seen"]:
                    c["status"] = 3
                    continue
                c["seen"].add(c["at"])
                nxt.append(i)
            act = nxt
        for c in chains:
            c.pop("at", None), c.pop("seen", None)
            if c["status"]:
                c.update(ind1=0, ind2=0, end_kmer=0, end_node=0, string="", distances=[], coverages=[], kills=[])
        return chains
