"""ContigGraph::removeChimerasAndClean (src/ContigGraph.cpp:177-184, removeChimericExtensions :642-707) on the graph deleteTipsAndClean left, and
printContigs behind it, restated in plain Python on top of tests/detip_plan_ref.py: what fgpu_chimera_plan (faucet_amd/csrc/tips_plan.cpp over
clean_graph.h) computes, written a second time, in another language and from the reference -- a contig here CARRIES ITS COVERAGE LIST, joined as
ContigJuncList::concatenate joins it (utils/ContigJuncList.cpp:107-123) and reversed as reverse does (:98-103), and getAvgCoverage (:162-172) sums
it; nothing is summarised.  For tests/test_dechimera_plan_cpu.py, tests/golden/make_chimera_golden.py and the command-line tests of
tests/test_gpu_dechimera.py.

The first step is tests/detip_plan_ref.plan itself; its outputs (the nodes in map order with their slots, the contig records with their ends, the
isolated contigs in the list's order) are the whole graph a later step can reach -- a contig in no slot that is not isolated is reached by nothing --
so the second step starts from them.

  getMinMaxForwardExtensions :295-320 (getIndicesOut src/ContigNode.cpp:227-235; std::minmax_element: the FIRST smallest, the LAST largest),
  indexOf src/ContigNode.cpp:266-274 (throws), cutPath :364-384, deleteContig :346-361, isCollapsible :617-640, collapseNode :1418-1467,
  validateNoneCollapsible :709-736 (only if a chimeric extension was counted), printContigs :1532-1645.

plan(...) -> (nodes, contigs, records, info, tips_info, averages): the first three in the terms of tests/detip_golden.Plan, info over
tests/dechimera_golden.INFO_KEYS, tips_info the first step's, averages[c] = getAvgCoverage of contig record c.  Unset as tests/detip_plan_ref."""
from tests import detip_plan_ref as R
from tests.detip_plan_ref import Unset

SKIP_NO_FAR, SKIP_BACK, SKIP_FAR_PATHS, SKIP_LONG, SKIP_RATIO, SKIP_OTHER_P = range(6)


class NoCoverage(Exception):
    """a contig of the build without a coverage entry: ContigJuncList::concatenate would read back() of an empty list"""


class _Tig(R._Tig):
    def __init__(self, pieces, length, node1, node2, ind1, ind2, cov):
        super().__init__(pieces, length, node1, node2, ind1, ind2)
        self.cov = list(cov)

    def reversed(self):
        return _Tig([(c, not f) for c, f in reversed(self.list)], self.len, self.node2, self.node1, self.ind2, self.ind1, self.cov[::-1])

    def avg(self):                                                            # getAvgCoverage: a double sum of the entries over their number
        total = 0.0
        for v in self.cov:
            total += float(v)
        return total / len(self.cov)


def _concatenated(left, right):                                               # ContigJuncList::concatenate on the coverages
    return left[:-1] + [min(left[-1], right[0])] + right[1:]


def _cov_of(pieces, call_covs):
    out = None
    for c, flip in pieces:
        own = call_covs[c][::-1] if flip else list(call_covs[c])
        if not own:
            raise NoCoverage(c)
        out = own if out is None else _concatenated(out, own)
    return out


class _Node:
    def __init__(self, cov, contigs):
        self.cov, self.contigs = list(cov), list(contigs)


def _ratio(a, b):                                                             # a / b as IEEE doubles divide
    if b == 0.0:
        return float("nan") if a == 0.0 else float("inf")
    return a / b


def plan(calls, keys, cov, k, read_length):
    call_covs = [list(w.contig.coverages) for w in calls]
    for c, v in enumerate(call_covs):
        if not v:
            raise NoCoverage(c)
    t_nodes, t_contigs, _, tips_info = R.plan(calls, keys, cov, k, read_length)
    tigs = [_Tig(p, n, n1, n2, i1, i2, _cov_of(p, call_covs)) for n1, n2, n, i1, i2, _, p in t_contigs]
    nodes = {key: _Node(ncov, [None if s < 0 else tigs[s] for s in slots]) for key, ncov, slots in t_nodes}
    isolated = [t for t, rec in zip(tigs, t_contigs) if rec[5]]
    info = dict(nodes_before=len(nodes), removed=0, cut_near=0, cut_far=0, cut_both=0, collapsed_0=0, collapsed_1=0, degenerate_0=0, degenerate_1=0,
                collapsed_after_cut=0, validated=0, changed=0)
    info.update({"skipped_%d" % i: 0 for i in range(6)})

    def node_at(key):
        if key not in nodes:
            raise Unset("a node that is gone: %x" % key)
        return nodes[key]

    def live(t):
        if t is None or not t.alive:
            raise Unset("a contig that is gone")
        return t

    def paths(nd):
        return sum(v > 0 for v in nd.cov)

    def index_of(nd, t):
        for i in range(5):
            if nd.contigs[i] is t:
                return i
        raise Unset("indexOf throws")

    def break_path(nd, i):
        if i > 4:
            raise Unset("index %d" % i)
        if i < 4:
            nd.cov[i] = 0
        nd.contigs[i] = None

    def cut_path(key, nd, i):
        if nd.contigs[i] is None:
            return
        t = live(nd.contigs[i])
        s = t.side_at(key, i)
        if t.node1 == t.node2:
            if s < 0:
                raise Unset("getIndex(4)")
            other_index = t.ind2 if s == 1 else t.ind1
            t.node1 = t.node2 = None
            break_path(nd, i)
            break_path(nd, other_index)
        else:
            if s == 1:
                t.node1 = None
            elif s == 2:
                t.node2 = None
            break_path(nd, i)

    def delete_contig(t):
        if t.node1 is not None:
            break_path(node_at(t.node1), t.ind1)
        if t.node2 is not None:
            break_path(node_at(t.node2), t.ind2)
        t.alive = False

    def is_collapsible(nd):
        if paths(nd) != 1 or nd.contigs[4] is None:
            return False
        front = next((t for t in nd.contigs[:4] if t is not None), None)
        if front is None:
            return False
        return not any(live(t).node1 is not None and t.node1 == t.node2 for t in (front, nd.contigs[4]))

    def collapse_node(key, nd):
        back = nd.contigs[4]
        fronts = [(i, t) for i, t in enumerate(nd.contigs[:4]) if t is not None]
        if back is None or not fronts:
            return
        fronti, front = fronts[-1]
        live(back), live(front)
        if front is back:
            isolated.append(_Tig(front.list, front.len, front.node1, front.node2, front.ind1, front.ind2, front.cov))
            back.alive = False
            return
        back_node, front_node = back.other(key), front.other(key)
        left = back.reversed() if back.side_at(key, 4) == 1 else back
        right = front.reversed() if front.side_at(key, fronti) == 2 else front
        made = _Tig(left.list + right.list, left.len - k + right.len, left.node1, right.node2, left.ind1, right.ind2, _concatenated(left.cov, right.cov))
        for at, index in ((made.node1, made.ind1), (made.node2, made.ind2), (back_node, made.ind1), (front_node, made.ind2)):
            if at is not None:
                if index > 4:
                    raise Unset("index %d" % index)
                node_at(at).contigs[index] = made
        if back_node is None and front_node is None:
            if made.node1 is not None or made.node2 is not None:
                raise Unset("a node keeps the deleted result")
            isolated.append(made)
        back.alive = front.alive = False

    def degenerate(key, nd):
        if paths(nd) == 0:
            if nd.contigs[4] is not None:
                cut_path(key, nd, 4)
            return True
        if nd.contigs[4] is None:
            for j in range(4):
                if nd.contigs[j] is not None:
                    cut_path(key, nd, j)
            return True
        return False

    def min_max(nd):
        inds = [i for i in range(4) if nd.cov[i] > 0]
        covs = [live(nd.contigs[i]).avg() for i in inds]
        lo = min(range(len(covs)), key=lambda j: (covs[j], j))                 # the first smallest
        hi = max(range(len(covs)), key=lambda j: (covs[j], j))                 # the last largest
        return nd.contigs[inds[lo]], nd.contigs[inds[hi]]

    for key in list(nodes):                                                   # removeChimericExtensions(150)
        nd = nodes[key]
        if paths(nd) > 1:
            p, q = min_max(nd)
            far = p.other(key)
            if far is None or far == key:
                info["skipped_%d" % SKIP_NO_FAR] += 1
                continue
            far_node = node_at(far)
            if index_of(far_node, p) == 4:
                info["skipped_%d" % SKIP_BACK] += 1
                continue
            if paths(far_node) < 2:
                info["skipped_%d" % SKIP_FAR_PATHS] += 1
                continue
            p2, q2 = min_max(far_node)
            ratio1, ratio2 = _ratio(q.avg(), p.avg()), _ratio(q2.avg(), p2.avg())
            if p.len < 150 and ratio1 >= 3 and p is p2:
                if ratio1 > ratio2:
                    cut_path(key, nd, index_of(nd, p))
                    info["cut_near"] += 1
                elif ratio2 > ratio1:
                    cut_path(far, far_node, index_of(far_node, p))
                    info["cut_far"] += 1
                else:
                    cut_path(key, nd, index_of(nd, p))
                    cut_path(far, far_node, index_of(far_node, p))
                    delete_contig(p)
                    info["cut_both"] += 1
                if is_collapsible(nd):
                    collapse_node(key, nd)
                    info["collapsed_0"] += 1
                    info["collapsed_after_cut"] += 1
                    del nodes[key]
                info["removed"] += 1
            else:
                info["skipped_%d" % (SKIP_LONG if not p.len < 150 else SKIP_RATIO if not ratio1 >= 3 else SKIP_OTHER_P)] += 1
        elif is_collapsible(nd):
            collapse_node(key, nd)
            info["collapsed_0"] += 1
            del nodes[key]
    info["changed"] = int(info["removed"] > 0)
    if info["changed"]:                                                       # validateNoneCollapsible
        info["validated"] = 1
        for key in list(nodes):
            nd = nodes[key]
            if paths(nd) == 0 and nd.contigs[4] is None:
                info["degenerate_1"] += 1
            elif is_collapsible(nd):
                collapse_node(key, nd)
                info["collapsed_1"] += 1
            elif degenerate(key, nd):
                info["degenerate_1"] += 1
            else:
                continue
            del nodes[key]
    records = []
    count = dict(bubble_records=0, node_contigs=0, isolated_kept=0, isolated_dropped=0)
    for key, nd in nodes.items():                                             # printAndMarkBubbleContigs
        out = [i for i in range(4) if nd.cov[i] > 0]
        if len(out) != 2:
            continue
        far = [live(nd.contigs[i]).other(key) for i in out]
        if far[0] != far[1] or far[0] is None:
            continue
        back = live(nd.contigs[4])
        if not back.len < 250:
            continue
        back_mark = False
        for i in range(4):
            t = nd.contigs[i]
            if t is None or live(t).mark:
                continue
            if not back.mark:
                left = back.reversed() if back.side(key) == 1 else back
                right = t.reversed() if t.side(key) == 2 else t
                records.append((len(records) + 1, left.list + right.list))
                count["bubble_records"] += 1
                back_mark = t.mark = True
        if back_mark:
            back.mark = True
    for key, nd in nodes.items():                                             # printUnmarkedUnitigs
        for t in nd.contigs:
            if t is None or live(t).mark:
                continue
            records.append((len(records) + 1, list(t.list)))
            count["node_contigs"] += 1
            t.mark = True
    for t in isolated:
        if t.len >= read_length:
            records.append((len(records) + 1, list(t.list)))
            count["isolated_kept"] += 1
        else:
            count["isolated_dropped"] += 1
    info.update(count, records=len(records), nodes=len(nodes))
    number, contigs, averages, out_nodes = {}, [], [], []

    def record(t, is_isolated):
        number[id(t)] = len(contigs)
        contigs.append((t.node1, t.node2, t.len, t.ind1, t.ind2, int(is_isolated), list(t.list)))
        averages.append(t.avg())

    for key, nd in nodes.items():
        slots = []
        for t in nd.contigs:
            if t is not None and id(t) not in number:
                record(t, False)
            slots.append(-1 if t is None else number[id(t)])
        out_nodes.append((key, list(nd.cov), slots))
    for t in isolated:
        record(t, True)
    return out_nodes, contigs, records, info, tips_info, averages
