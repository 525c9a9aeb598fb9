"""ContigGraph::deleteTipsAndClean (src/ContigGraph.cpp:168-175) on the graph JunctionMap::buildContigGraph returns, and printContigs behind it,
restated in plain Python over the structures of tests/graph_build_ref.py and tests/raw_contigs_ref.py: what fgpu_tips_plan
(faucet_amd/csrc/tips_plan.cpp) computes, written a second time and in another language, for tests/test_detip_plan_cpu.py and the command-line tests
of tests/test_gpu_detip.py.  The text of a contig is tests/detip_ref.join's.

A contig is a _Tig: its piece list [(call, flip)], its joined length (the sum of the pieces' lengths minus (pieces - 1) k), node1 / node2 (keys of
nodeMap or None) and ind1 / ind2.  The map is gone over in the order tests/raw_contigs_ref.graph_of gives (the container's, replayed by
tests/dump_order_ref.py); an erased node leaves the order of the others as it is.

  deleteTips :575-615, isTip :324-330, cutPath :364-384, deleteContig :346-361, breakPath src/ContigNode.cpp:280-283 (cov has four entries),
  isCollapsible :617-640 (the FIRST front contig), collapseNode :1418-1467 (the LAST), Contig::concatenate src/Contig.cpp:83-109,
  testAndCutIfDegenerate :403-425, validateNoneCollapsible :709-736 (only if deleteTips counted a tip), printContigs :1532-1645.

plan(...) -> (nodes, contigs, records, info) in the terms of tests/detip_golden.Plan; Unset: the reference would go through a pointer nobody set, or
to a node or contig that is gone."""
from tests import raw_contigs_ref as P


class Unset(Exception):
    pass


class _Tig:
    def __init__(self, pieces, length, node1=None, node2=None, ind1=5, ind2=5):
        self.list, self.len, self.node1, self.node2, self.ind1, self.ind2 = list(pieces), length, node1, node2, ind1, ind2
        self.mark, self.alive = False, True

    def reversed(self):                                                       # Contig::reverse, on a copy
        return _Tig([(c, not f) for c, f in reversed(self.list)], self.len, self.node2, self.node1, self.ind2, self.ind1)

    def side_at(self, node, index):                                           # Contig::getSide(node, index)
        if self.node1 == node and self.ind1 == index:
            return 1
        return 2 if self.node2 == node and self.ind2 == index else -1

    def side(self, node):                                                     # Contig::getSide(node)
        return 1 if self.node1 == node else 2 if self.node2 == node else -1

    def other(self, node):                                                    # Contig::otherEndNode
        return self.node2 if self.node1 == node else self.node1 if self.node2 == node else None


def plan(calls, keys, cov, k, read_length):
    order, ends, linear = P.graph_of(calls, keys, cov, k)
    nodes = dict(order)                                                       # (insertion-ordered: the container's order; del keeps the rest)
    tigs = [_Tig([(c, False)], len(w.contig.string), ends[c].node1, ends[c].node2, w.contig.ind1, w.contig.ind2) for c, w in enumerate(calls)]
    for nd in nodes.values():
        nd.contigs = [None if c is None else tigs[c] for c in nd.contigs]
    isolated = []
    for b, f in linear:                                                       # backward->concatenate(forward, 1, 1)
        left = tigs[b].reversed()
        isolated.append(_Tig(left.list + tigs[f].list, left.len - k + tigs[f].len, None, None, left.ind1, tigs[f].ind2))
    info = dict(nodes_before=len(nodes), tips=0, back_tips=0, collapsed_0=0, collapsed_1=0, degenerate_0=0, degenerate_1=0, validated=0, changed=0)

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

    def break_path(nd, i):
        if i > 4:
            raise Unset("index %d" % i)
        if i < 4:
            nd.cov[i] = 0
        nd.contigs[i] = None

    def is_tip(key, nd, i):
        t = live(nd.contigs[i])
        return t.len < read_length and t.other(key) in (None, key)             # (the reference's int goes to unsigned: read_length >= 0 here)

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
            copy = _Tig(front.list, front.len, front.node1, front.node2, front.ind1, front.ind2)
            isolated.append(copy)
            back.alive = False
            return
        back_node, front_node = back.other(key), front.other(key)
        left = back.reversed() if back.side_at(key, 4) == 1 else back
        right = front.reversed() if front.side_at(key, fronti) == 2 else front
        made = _Tig(left.list + right.list, left.len - k + right.len, left.node1, right.node2, left.ind1, right.ind2)
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

    for key in list(nodes):                                                   # deleteTips
        nd = nodes[key]
        for i in range(4):
            t = nd.contigs[i]
            if t is not None and is_tip(key, nd, i) and paths(nd) > 1:
                cut_path(key, nd, i)
                delete_contig(t)
                info["tips"] += 1
        if nd.contigs[4] is not None and is_tip(key, nd, 4):
            t = nd.contigs[4]
            cut_path(key, nd, 4)
            delete_contig(t)
            info["back_tips"] += 1
        if is_collapsible(nd):
            collapse_node(key, nd)
            info["collapsed_0"] += 1
            del nodes[key]
        elif degenerate(key, nd):
            info["degenerate_0"] += 1
            del nodes[key]
    info["changed"] = int(info["tips"] > 0)
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
    number, contigs, out_nodes = {}, [], []

    def record(t, is_isolated):
        number[id(t)] = len(contigs)
        contigs.append((t.node1, t.node2, t.len, t.ind1, t.ind2, int(is_isolated), list(t.list)))

    for key, nd in nodes.items():
        slots = []
        for t in nd.contigs:
            if t is not None and id(t) not in number:
                record(t, False)
            slots.append(-1 if t is None else number[id(t)])
        out_nodes.append((key, list(nd.cov), slots))
    for t in isolated:
        record(t, True)
    return out_nodes, contigs, records, info
