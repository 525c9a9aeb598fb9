// tips_plan.cpp — which piece lists ContigGraph::deleteTipsAndClean leaves of a build's contigs, and which of them printContigs prints: host
// logic only (no HIP, no text, no coverage list), so that a stand-alone CPU program can compile it in (tests/host/tips_plan_check.cpp, under the
// sanitizers).  The graph is build_graph.h's; a contig here is a list of (call, flip) and its two ends.
//   deleteTipsAndClean, deleteTips, isTip          src/ContigGraph.cpp:168-175, :575-615, :324-330
//   cutPath, deleteContig, breakPath               src/ContigGraph.cpp:364-384, :346-361, src/ContigNode.cpp:280-283 (cov has four entries)
//   isCollapsible, collapseNode                    src/ContigGraph.cpp:617-640, :1418-1467
//   Contig::concatenate, reverse, setEnds          src/Contig.cpp:83-109, :111-121, :123-133
//   Contig::getSide(node, index), otherEndNode     src/Contig.cpp:255-265, :182-193
//   testAndCutIfDegenerate                         src/ContigGraph.cpp:403-425
//   validateNoneCollapsible                        src/ContigGraph.cpp:709-736
//   printAndMarkBubbleContigs, printUnmarkedUnitigs  src/ContigGraph.cpp:1543-1580, :1605-1645 (as raw_plan.cpp walks them)
// Wherever the reference would go through a pointer to a node that was erased or a contig that was deleted, or with an index that is none,
// the answer is FGPU_PLAN_UNSET.
#include <cstdint>
#include <cstring>
#include <vector>

#include "build_graph.h"

namespace {

using namespace fgpu_graph;

struct Tig {                 // a Contig: its piece list, joined length, ends and indices
    std::vector<fgpu_join_piece> list;
    uint64_t len = 0, node1 = 0, node2 = 0;
    bool has1 = false, has2 = false, mark = false, alive = true;
    int ind1 = 5, ind2 = 5;  // (Contig::Contig(): 5)
};

struct End {
    bool has;
    uint64_t key;
};

void reverse(Tig& t) {       // Contig::reverse: the ends and indices swapped, the list reversed and every flip toggled
    std::swap(t.node1, t.node2);
    std::swap(t.has1, t.has2);
    std::swap(t.ind1, t.ind2);
    std::vector<fgpu_join_piece> r(t.list.rbegin(), t.list.rend());
    for (auto& p : r) p.flip ^= 1u;
    t.list.swap(r);
}

struct Cleaner {
    std::unordered_map<uint64_t, Node>& node_map;
    std::vector<Tig> tigs;
    std::vector<int64_t> isolated;       // isolated_contigs, as numbers of tigs
    int32_t k, read_length;
    bool unset = false;

    Cleaner(std::unordered_map<uint64_t, Node>& m, int32_t k_, int32_t rl) : node_map(m), k(k_), read_length(rl) {}

    Node* node_at(uint64_t key) {        // a ContigNode* that is followed
        auto at = node_map.find(key);
        if (at == node_map.end()) { unset = true; return nullptr; }
        return &at->second;
    }
    Tig* tig_at(int64_t t) {             // a Contig* that is followed
        if (t == NONE || !tigs[t].alive) { unset = true; return nullptr; }
        return &tigs[t];
    }
    static int paths_out(const Node& nd) {
        int n = 0;
        for (int i = 0; i < 4; i++) n += nd.cov[i] > 0;
        return n;
    }
    static void break_path(Node& nd, int i) {
        if (i < 4) nd.cov[i] = 0;
        nd.contigs[i] = NONE;
    }
    static int side_at(const Tig& t, uint64_t node, int index) {      // Contig::getSide(node, index)
        if (t.has1 && t.node1 == node && t.ind1 == index) return 1;
        if (t.has2 && t.node2 == node && t.ind2 == index) return 2;
        return -1;
    }
    static int side(const Tig& t, uint64_t node) {                    // Contig::getSide(node)
        if (t.has1 && t.node1 == node) return 1;
        if (t.has2 && t.node2 == node) return 2;
        return -1;
    }
    static End other_end(const Tig& t, uint64_t node) {               // Contig::otherEndNode
        if (t.has1 && t.node1 == node) return End{t.has2, t.node2};
        if (t.has2 && t.node2 == node) return End{t.has1, t.node1};
        return End{false, 0};
    }
    static bool same_ends(const Tig& t) { return t.has1 == t.has2 && (!t.has1 || t.node1 == t.node2); }      // node1_p == node2_p

    bool is_tip(uint64_t node, Node& nd, int i) {
        Tig* t = tig_at(nd.contigs[i]);
        if (!t) return false;
        const End far = other_end(*t, node);
        return t->len < (uint64_t)(int64_t)read_length && (!far.has || far.key == node);
    }
    void cut_path(uint64_t node, Node& nd, int index) {
        if (nd.contigs[index] == NONE) return;
        Tig* t = tig_at(nd.contigs[index]);
        if (!t) return;
        const int s = side_at(*t, node, index);
        if (same_ends(*t)) {
            if (s < 0) { unset = true; return; }                     // getIndex(4) throws
            const int other_index = s == 1 ? t->ind2 : t->ind1;
            if (other_index > 4) { unset = true; return; }
            t->has1 = t->has2 = false;
            break_path(nd, index);
            break_path(nd, other_index);
        } else {
            if (s == 1) t->has1 = false;
            if (s == 2) t->has2 = false;
            break_path(nd, index);
        }
    }
    void delete_contig(int64_t c) {
        Tig& t = tigs[c];
        if (t.has1) { Node* n = node_at(t.node1); if (!n || t.ind1 > 4) { unset = true; return; } break_path(*n, t.ind1); }
        if (t.has2) { Node* n = node_at(t.node2); if (!n || t.ind2 > 4) { unset = true; return; } break_path(*n, t.ind2); }
        t.alive = false;
    }
    bool is_collapsible(Node& nd) {
        if (paths_out(nd) != 1 || nd.contigs[4] == NONE) return false;
        int64_t front = NONE;
        for (int i = 0; i < 4 && front == NONE; i++) front = nd.contigs[i];
        if (front == NONE) return false;
        const Tig *f = tig_at(front), *b = tig_at(nd.contigs[4]);
        if (!f || !b) return false;
        if (f->has1 && f->has2 && f->node1 == f->node2) return false;
        if (b->has1 && b->has2 && b->node1 == b->node2) return false;
        return true;
    }
    void collapse_node(uint64_t node, Node& nd) {
        const int64_t back = nd.contigs[4];
        if (back == NONE) return;
        int64_t front = NONE;
        int fronti = 0;
        for (int i = 0; i < 4; i++)
            if (nd.contigs[i] != NONE) { front = nd.contigs[i]; fronti = i; }
        if (front == NONE) return;
        if (!tig_at(back) || !tig_at(front)) return;
        if (front == back) {                                         // (a copy goes to isolated_contigs, its ends as they are)
            Tig copy = tigs[front];
            tigs.push_back(copy);
            isolated.push_back((int64_t)tigs.size() - 1);
            tigs[back].alive = false;
            return;
        }
        const End back_node = other_end(tigs[back], node), front_node = other_end(tigs[front], node);
        const int back_side = side_at(tigs[back], node, 4), front_side = side_at(tigs[front], node, fronti);
        Tig left = tigs[back], right = tigs[front];
        if (back_side == 1) reverse(left);
        if (front_side == 2) reverse(right);
        Tig made;
        made.node1 = left.node1; made.has1 = left.has1; made.ind1 = left.ind1;
        made.node2 = right.node2; made.has2 = right.has2; made.ind2 = right.ind2;
        made.list = left.list;
        made.list.insert(made.list.end(), right.list.begin(), right.list.end());
        made.len = left.len - (uint64_t)k + right.len;
        tigs.push_back(made);
        const int64_t m = (int64_t)tigs.size() - 1;
        auto store = [&](bool has, uint64_t key, int index) {
            if (!has) return;
            Node* n = node_at(key);
            if (!n || index > 4) { unset = true; return; }
            n->contigs[index] = m;
        };
        store(made.has1, made.node1, made.ind1);                     // setEnds
        store(made.has2, made.node2, made.ind2);
        store(back_node.has, back_node.key, made.ind1);
        store(front_node.has, front_node.key, made.ind2);
        if (!back_node.has && !front_node.has) {
            if (made.has1 || made.has2) unset = true;                // (a node would keep a pointer to the deleted result)
            isolated.push_back(m);
        }
        tigs[back].alive = false;
        tigs[front].alive = false;
    }
    bool test_and_cut_if_degenerate(uint64_t node, Node& nd) {
        const int paths = paths_out(nd);
        if (paths == 0) {
            if (nd.contigs[4] != NONE) cut_path(node, nd, 4);
            return true;
        }
        if (nd.contigs[4] == NONE) {
            for (int j = 0; j < 4; j++)
                if (nd.contigs[j] != NONE) cut_path(node, nd, j);
            return true;
        }
        return false;
    }
};

template <class T>
struct Room {                // an output array: written while there is room, counted always
    T* out;
    uint64_t cap, n = 0;
    Room(T* o, uint64_t c) : out(o), cap(o ? c : 0) {}
    void put(const T& v) { if (n < cap) out[n] = v; n++; }
};

}  // namespace

extern "C" int fgpu_tips_plan(const uint64_t* keys, const fgpu_junction* recs, uint64_t n_junctions, const fgpu_contig* contigs, const fgpu_build_call* calls,
                              uint64_t n_calls, int32_t k, int32_t read_length, fgpu_tips_out* out, fgpu_tips_info* info) {
    if (!out) return FGPU_PLAN_INPUT;
    out->n_nodes = out->n_contigs = out->n_pieces = out->n_print = out->n_print_pieces = 0;
    if ((out->contigs_cap && out->contigs && !out->list_first) || (out->print_cap && out->print_number && !out->print_first)) return FGPU_PLAN_INPUT;
    Graph g;
    if (int st = of_build(keys, recs, n_junctions, contigs, calls, n_calls, k, g)) return st;
    Cleaner cl(g.node_map, k, read_length);
    cl.tigs.resize(n_calls);
    for (uint64_t c = 0; c < n_calls; c++) {
        Tig& t = cl.tigs[c];
        t.list.push_back(fgpu_join_piece{(uint32_t)c, 0});
        t.len = contigs[c].len;
        t.node1 = g.ends[c].node1; t.has1 = g.ends[c].has1; t.ind1 = contigs[c].ind1;
        t.node2 = g.ends[c].node2; t.has2 = g.ends[c].has2; t.ind2 = contigs[c].ind2;
        t.alive = calls[c].phase == FGPU_BUILD_BRANCHING;            // (the two chains of a linear region are deleted behind their join)
    }
    for (uint64_t f : g.isolated) {                                  // backward->concatenate(forward, 1, 1)
        Tig left = cl.tigs[f + 1], made;
        reverse(left);
        made.ind1 = left.ind1; made.ind2 = cl.tigs[f].ind2;
        made.list = left.list;
        made.list.push_back(fgpu_join_piece{(uint32_t)f, 0});
        made.len = left.len - (uint64_t)k + cl.tigs[f].len;
        cl.tigs.push_back(made);
        cl.isolated.push_back((int64_t)cl.tigs.size() - 1);
    }
    fgpu_tips_info inf;
    memset(&inf, 0, sizeof(inf));
    inf.nodes_before = g.node_map.size();
    // ---- deleteTips
    for (auto it = g.node_map.begin(); it != g.node_map.end();) {
        const uint64_t node = it->first;
        Node& nd = it->second;
        for (int i = 0; i < 4; i++) {
            const int64_t c = nd.contigs[i];
            if (c == NONE) continue;
            if (cl.is_tip(node, nd, i) && Cleaner::paths_out(nd) > 1) {
                cl.cut_path(node, nd, i);
                cl.delete_contig(c);
                inf.tips++;
            }
            if (cl.unset) return FGPU_PLAN_UNSET;
        }
        if (nd.contigs[4] != NONE && cl.is_tip(node, nd, 4)) {
            const int64_t c = nd.contigs[4];
            cl.cut_path(node, nd, 4);
            cl.delete_contig(c);
            inf.back_tips++;
        }
        bool erase = false;
        if (!cl.unset && cl.is_collapsible(nd)) {
            cl.collapse_node(node, nd);
            inf.collapsed[0]++;
            erase = true;
        } else if (!cl.unset && cl.test_and_cut_if_degenerate(node, nd)) {
            inf.degenerate[0]++;
            erase = true;
        }
        if (cl.unset) return FGPU_PLAN_UNSET;
        if (erase) it = g.node_map.erase(it); else ++it;
    }
    inf.changed = inf.tips > 0;
    // ---- validateNoneCollapsible
    if (inf.changed) {
        inf.validated = 1;
        for (auto it = g.node_map.begin(); it != g.node_map.end();) {
            const uint64_t node = it->first;
            Node& nd = it->second;
            bool erase = false;
            if (Cleaner::paths_out(nd) == 0 && nd.contigs[4] == NONE) {
                inf.degenerate[1]++;
                erase = true;
            } else if (cl.is_collapsible(nd)) {
                cl.collapse_node(node, nd);
                inf.collapsed[1]++;
                erase = true;
            } else if (!cl.unset && cl.test_and_cut_if_degenerate(node, nd)) {
                inf.degenerate[1]++;
                erase = true;
            }
            if (cl.unset) return FGPU_PLAN_UNSET;
            if (erase) it = g.node_map.erase(it); else ++it;
        }
    }
    std::vector<Tig>& tigs = cl.tigs;
    Room<uint64_t> print_first(out->print_first, out->print_first ? out->print_cap + 1 : 0);
    Room<uint32_t> print_number(out->print_number, out->print_cap);
    Room<fgpu_join_piece> print_pieces(out->print_pieces, out->print_pieces_cap);
    auto print = [&](const std::vector<fgpu_join_piece>& a, const std::vector<fgpu_join_piece>* b) {
        print_first.put(print_pieces.n);
        print_number.put((uint32_t)(print_number.n + 1));
        for (const auto& p : a) print_pieces.put(p);
        if (b) for (const auto& p : *b) print_pieces.put(p);
    };
    // ---- printAndMarkBubbleContigs
    fgpu_raw_info& pr = inf.print;
    pr.nodes = g.node_map.size();
    for (auto& kv : g.node_map) {
        const uint64_t node = kv.first;
        Node& nd = kv.second;
        if (Cleaner::paths_out(nd) != 2) continue;                   // isBubbleNode
        bool first_far = true, same = true;
        End far0 = {false, 0};
        for (int i = 0; i < 4; i++) {
            if (!(nd.cov[i] > 0)) continue;
            const Tig* t = cl.tig_at(nd.contigs[i]);
            if (!t) return FGPU_PLAN_UNSET;                          // tig->otherEndNode(node) on a null tig
            const End far = Cleaner::other_end(*t, node);
            if (first_far) { far0 = far; first_far = false; }
            else same = far.has == far0.has && (!far.has || far.key == far0.key);
        }
        if (!same || !far0.has) continue;                            // allSame (:153-162): two null nodes are not the same
        if (!cl.tig_at(nd.contigs[4])) return FGPU_PLAN_UNSET;       // back->getSeq() on a null back
        const int64_t back = nd.contigs[4];
        if (!(tigs[back].len < 250)) continue;
        bool back_mark = false;
        for (int i = 0; i < 4; i++) {
            const int64_t c = nd.contigs[i];
            if (c == NONE) continue;
            if (!cl.tig_at(c)) return FGPU_PLAN_UNSET;
            if (tigs[c].mark) continue;
            if (!tigs[back].mark) {
                Tig left = tigs[back], right = tigs[c];
                if (Cleaner::side(left, node) == 1) reverse(left);
                if (Cleaner::side(right, node) == 2) reverse(right);
                print(left.list, &right.list);
                pr.bubble_records++;
                back_mark = true;
                tigs[c].mark = true;
            }
        }
        if (back_mark) tigs[back].mark = true;
    }
    // ---- printUnmarkedUnitigs
    for (auto& kv : g.node_map) {
        Node& nd = kv.second;
        for (int i = 0; i < 5; i++) {
            const int64_t c = nd.contigs[i];
            if (c == NONE) continue;
            if (!cl.tig_at(c)) return FGPU_PLAN_UNSET;
            if (tigs[c].mark) continue;
            print(tigs[c].list, nullptr);
            pr.node_contigs++;
            tigs[c].mark = true;
        }
    }
    for (int64_t c : cl.isolated) {
        if (tigs[c].len >= (uint64_t)(int64_t)read_length) {         // (size_t >= int: the int goes to unsigned)
            print(tigs[c].list, nullptr);
            pr.isolated_kept++;
        } else {
            pr.isolated_dropped++;
        }
    }
    print_first.put(print_pieces.n);
    pr.records = print_number.n;
    // ---- the graph left
    Room<fgpu_tips_node> nodes(out->nodes, out->nodes_cap);
    Room<fgpu_tips_contig> recs_out(out->contigs, out->contigs_cap);
    Room<uint64_t> list_first(out->list_first, out->list_first ? out->contigs_cap + 1 : 0);
    Room<fgpu_join_piece> pieces(out->pieces, out->pieces_cap);
    std::vector<int64_t> number(tigs.size(), NONE);
    auto record = [&](int64_t c, bool is_isolated) {
        const Tig& t = tigs[c];
        fgpu_tips_contig r;
        memset(&r, 0, sizeof(r));
        r.node1 = t.has1 ? t.node1 : 0; r.node2 = t.has2 ? t.node2 : 0;
        r.has1 = t.has1; r.has2 = t.has2; r.ind1 = (uint8_t)t.ind1; r.ind2 = (uint8_t)t.ind2;
        r.len = (uint32_t)t.len; r.isolated = is_isolated;
        number[c] = (int64_t)recs_out.n;
        recs_out.put(r);
        list_first.put(pieces.n);
        for (const auto& p : t.list) pieces.put(p);
    };
    for (auto& kv : g.node_map) {
        fgpu_tips_node n;
        memset(&n, 0, sizeof(n));
        n.key = kv.first;
        for (int i = 0; i < 4; i++) n.cov[i] = kv.second.cov[i];
        for (int i = 0; i < 5; i++) {
            const int64_t c = kv.second.contigs[i];
            if (c != NONE && number[c] == NONE) record(c, false);
            n.slot[i] = c == NONE ? -1 : (int32_t)number[c];
        }
        nodes.put(n);
    }
    for (int64_t c : cl.isolated) record(c, true);
    list_first.put(pieces.n);
    out->n_nodes = nodes.n; out->n_contigs = recs_out.n; out->n_pieces = pieces.n; out->n_print = print_number.n; out->n_print_pieces = print_pieces.n;
    if (info) *info = inf;
    const bool fits = (!nodes.n || nodes.n <= nodes.cap) && (!recs_out.n || (recs_out.n <= recs_out.cap && list_first.n <= list_first.cap)) &&
                      (!pieces.n || pieces.n <= pieces.cap) && (!print_number.n || (print_number.n <= print_number.cap && print_first.n <= print_first.cap)) &&
                      (!print_pieces.n || print_pieces.n <= print_pieces.cap);
    return fits ? FGPU_PLAN_OK : FGPU_PLAN_SHORT;
}
