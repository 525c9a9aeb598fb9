// clean_graph.h — the reference's ContigGraph while ContigGraph::cleanGraph works on it, over piece lists instead of strings: host logic only (no
// HIP, no text, no coverage list), so that a stand-alone CPU program can compile it in (tests/host/tips_plan_check.cpp and
// chimera_plan_check.cpp, under the sanitizers).  One object owns nodeMap -- build_graph.h's, a real std::unordered_map that took the reference's
// inserts and takes its erases --, the contigs and isolated_contigs, and lives from step to step: nothing is made again between two steps.  A
// contig is a list of (call, flip) over the calls of the build, its two ends, and the summary of its coverage list (cov_summary.h).
//   deleteTipsAndClean, deleteTips, isTip          src/ContigGraph.cpp:168-175, :575-615, :324-330
//   removeChimerasAndClean, removeChimericExtensions   src/ContigGraph.cpp:177-184, :642-707
//   getMinMaxForwardExtensions                     src/ContigGraph.cpp:295-320; ContigNode::getIndicesOut, indexOf src/ContigNode.cpp:227-235, :266-274
//   cutPath, deleteContig, breakPath               src/ContigGraph.cpp:364-384, :346-361, src/ContigNode.cpp:280-283 (cov has four entries)
//   isCollapsible, collapseNode                    src/ContigGraph.cpp:617-640, :1418-1467
//   Contig::concatenate, reverse, setEnds          src/Contig.cpp:83-109, :111-121, :123-133
//   Contig::getSide(node, index), otherEndNode     src/Contig.cpp:255-265, :182-193
//   Contig::getAvgCoverage                         src/Contig.cpp:153-155, utils/ContigJuncList.cpp:162-172
//   testAndCutIfDegenerate                         src/ContigGraph.cpp:403-425
//   validateNoneCollapsible                        src/ContigGraph.cpp:709-736
//   printAndMarkBubbleContigs, printUnmarkedUnitigs  src/ContigGraph.cpp:1543-1580, :1605-1645 (as raw_plan.cpp walks them)
//   printGraph, ContigIterator                     src/ContigGraph.cpp:1470-1503, src/ContigIterator.cpp
//   Contig::getNeighbors, getFastGNeighbors        src/Contig.cpp:290-302, src/ContigNode.cpp:179-202
// Wherever the reference would go through a pointer to a node that was erased or a contig that was deleted, or with an index that is none,
// the answer is FGPU_PLAN_UNSET.
#ifndef FGPU_CLEAN_GRAPH_H
#define FGPU_CLEAN_GRAPH_H
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

#include "build_graph.h"
#include "cov_summary.h"

namespace fgpu_graph {

struct Tig {                 // a Contig: its piece list, joined length, ends and indices, and what its coverage list comes to
    std::vector<fgpu_join_piece> list;
    uint64_t len = 0, node1 = 0, node2 = 0;
    bool has1 = false, has2 = false, alive = true;
    int ind1 = 5, ind2 = 5;  // (Contig::Contig(): 5)
    fgpu_cov_summary cov = {0, 0, 0, 0, {0, 0}};     // (all 0 until the graph is given the calls' summaries)
};

struct End {
    bool has;
    uint64_t key;
};

inline void reverse(Tig& t) {       // Contig::reverse: the ends and indices swapped, the list reversed and every flip toggled
    std::swap(t.node1, t.node2);
    std::swap(t.has1, t.has2);
    std::swap(t.ind1, t.ind2);
    std::vector<fgpu_join_piece> r(t.list.rbegin(), t.list.rend());
    for (auto& p : r) p.flip ^= 1u;
    t.list.swap(r);
    t.cov = fgpu_cov_reverse(t.cov);
}

template <class T>
struct Room {                // an output array: written while there is room, counted always
    T* out;
    uint64_t cap, n = 0;
    Room(T* o, uint64_t c) : out(o), cap(o ? c : 0) {}
    void put(const T& v) { if (n < cap) out[n] = v; n++; }
    bool fits() const { return !n || n <= cap; }
};

struct FastgPlan {            // what ContigGraph::printGraph writes, in file order (CleanGraph::fastg_records)
    std::vector<int64_t> tig;            // per record: the contig, as a number of CleanGraph::tigs (its piece list, length and summary are there)
    std::vector<uint64_t> nbr_first;     // 2 records + 1: the neighbours of record r's primed header are nbr[nbr_first[2r] .. nbr_first[2r + 1]),
    std::vector<uint32_t> nbr;           // those of its other header nbr[nbr_first[2r + 1] .. nbr_first[2r + 2]); an entry: record | FGPU_FASTG_PRIMED
    fgpu_fastg_info info = {0, 0, 0, 0};
};

struct CleanGraph {
    Graph g;                             // nodeMap; what else it holds is read by of_build()
    std::vector<Tig> tigs;
    std::vector<int64_t> isolated;       // isolated_contigs, as numbers of tigs
    int32_t k = 0, read_length = 0;
    bool unset = false, have_cov = false;

    // ---- the graph JunctionMap::buildContigGraph returns.  cov_calls: one summary per call, or null (the graph then knows no coverage until
    // set_cov).  FGPU_PLAN_OK or FGPU_PLAN_INPUT.
    int of_build(const uint64_t* keys, const fgpu_junction* recs, uint64_t n_junctions, const fgpu_contig* contigs, const fgpu_build_call* calls, uint64_t n_calls,
                 const fgpu_cov_summary* cov_calls, int32_t k_, int32_t read_length_) {
        k = k_; read_length = read_length_;
        if (int st = fgpu_graph::of_build(keys, recs, n_junctions, contigs, calls, n_calls, k, g)) return st;
        have_cov = cov_calls != nullptr;
        for (uint64_t c = 0; have_cov && c < n_calls; c++)
            if (cov_calls[c].n == 0) return FGPU_PLAN_INPUT;         // (ContigJuncList::concatenate reads back() of an empty list)
        tigs.resize(n_calls);
        for (uint64_t c = 0; c < n_calls; c++) {
            Tig& t = tigs[c];
            t.list.push_back(fgpu_join_piece{(uint32_t)c, 0});
            t.len = contigs[c].len;
            t.node1 = g.ends[c].node1; t.has1 = g.ends[c].has1; t.ind1 = contigs[c].ind1;
            t.node2 = g.ends[c].node2; t.has2 = g.ends[c].has2; t.ind2 = contigs[c].ind2;
            t.alive = calls[c].phase == FGPU_BUILD_BRANCHING;        // (the two chains of a linear region are deleted behind their join)
            if (have_cov) t.cov = cov_calls[c];
        }
        for (uint64_t f : g.isolated) {                              // backward->concatenate(forward, 1, 1)
            Tig left = tigs[f + 1], made;
            reverse(left);
            made.ind1 = left.ind1; made.ind2 = tigs[f].ind2;
            made.list = left.list;
            made.list.push_back(fgpu_join_piece{(uint32_t)f, 0});
            made.len = left.len - (uint64_t)k + tigs[f].len;
            if (have_cov) made.cov = fgpu_cov_concatenate(left.cov, tigs[f].cov);
            tigs.push_back(made);
            isolated.push_back((int64_t)tigs.size() - 1);
        }
        return FGPU_PLAN_OK;
    }

    // ---- a graph that was made and cleaned without coverages is given them: every contig's summary is the fold over its piece list, which
    // is what the joins that made it would have folded (the operation is associative).  FGPU_PLAN_OK or FGPU_PLAN_INPUT.
    int set_cov(const fgpu_cov_summary* cov_calls, uint64_t n_calls) {
        for (uint64_t c = 0; c < n_calls; c++)
            if (cov_calls[c].n == 0) return FGPU_PLAN_INPUT;
        for (Tig& t : tigs) {
            if (!t.alive) continue;                                  // (nothing reads a deleted contig's summary: tig_at refuses it)
            bool first = true;
            for (const fgpu_join_piece& p : t.list) {
                if (p.call >= n_calls) return FGPU_PLAN_INPUT;
                const fgpu_cov_summary s = p.flip ? fgpu_cov_reverse(cov_calls[p.call]) : cov_calls[p.call];
                t.cov = first ? s : fgpu_cov_concatenate(t.cov, s);
                first = false;
            }
        }
        have_cov = true;
        return FGPU_PLAN_OK;
    }

    Node* node_at(uint64_t key) {        // a ContigNode* that is followed
        auto at = g.node_map.find(key);
        if (at == g.node_map.end()) { unset = true; return nullptr; }
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
    int index_of(const Node& nd, int64_t c) {                         // ContigNode::indexOf: throws where the contig is not there
        for (int i = 0; i < 5; i++)
            if (nd.contigs[i] == c) return i;
        unset = true;
        return -1;
    }

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
        if (have_cov) made.cov = fgpu_cov_concatenate(left.cov, right.cov);     // (after the same reversals as the lists)
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

    // ---- validateNoneCollapsible: FGPU_PLAN_OK or FGPU_PLAN_UNSET
    int validate_none_collapsible(uint64_t& collapsed, uint64_t& degenerate) {
        for (auto it = g.node_map.begin(); it != g.node_map.end();) {
            const uint64_t node = it->first;
            Node& nd = it->second;
            bool erase = false;
            if (paths_out(nd) == 0 && nd.contigs[4] == NONE) {
                degenerate++;
                erase = true;
            } else if (is_collapsible(nd)) {
                collapse_node(node, nd);
                collapsed++;
                erase = true;
            } else if (!unset && test_and_cut_if_degenerate(node, nd)) {
                degenerate++;
                erase = true;
            }
            if (unset) return FGPU_PLAN_UNSET;
            if (erase) it = g.node_map.erase(it); else ++it;
        }
        return FGPU_PLAN_OK;
    }

    // ---- deleteTipsAndClean: FGPU_PLAN_OK or FGPU_PLAN_UNSET; inf.print is not touched
    int delete_tips_and_clean(fgpu_tips_info& inf) {
        inf.nodes_before = g.node_map.size();
        for (auto it = g.node_map.begin(); it != g.node_map.end();) {          // deleteTips
            const uint64_t node = it->first;
            Node& nd = it->second;
            for (int i = 0; i < 4; i++) {
                const int64_t c = nd.contigs[i];
                if (c == NONE) continue;
                if (is_tip(node, nd, i) && paths_out(nd) > 1) {
                    cut_path(node, nd, i);
                    delete_contig(c);
                    inf.tips++;
                }
                if (unset) return FGPU_PLAN_UNSET;
            }
            if (nd.contigs[4] != NONE && is_tip(node, nd, 4)) {
                const int64_t c = nd.contigs[4];
                cut_path(node, nd, 4);
                delete_contig(c);
                inf.back_tips++;
            }
            bool erase = false;
            if (!unset && is_collapsible(nd)) {
                collapse_node(node, nd);
                inf.collapsed[0]++;
                erase = true;
            } else if (!unset && test_and_cut_if_degenerate(node, nd)) {
                inf.degenerate[0]++;
                erase = true;
            }
            if (unset) return FGPU_PLAN_UNSET;
            if (erase) it = g.node_map.erase(it); else ++it;
        }
        inf.changed = inf.tips > 0;
        if (inf.changed) {
            inf.validated = 1;
            return validate_none_collapsible(inf.collapsed[1], inf.degenerate[1]);
        }
        return FGPU_PLAN_OK;
    }

    // getMinMaxForwardExtensions(node, "coverage"): over getIndicesOut() -- the indices with cov > 0, in order -- the contig of the FIRST
    // smallest and of the LAST largest average (std::minmax_element).  false: a covered slot has no contig
    bool min_max_coverage(Node& nd, int64_t& lowest, int64_t& highest) {
        int inds[4], n = 0;
        std::vector<double> covs;
        for (int i = 0; i < 4; i++) {
            if (!(nd.cov[i] > 0)) continue;
            const Tig* t = tig_at(nd.contigs[i]);                    // node->contigs[inds[i]]->otherEndNode(node) on a null tig
            if (!t) return false;
            inds[n++] = i;
            covs.push_back(fgpu_cov_average(t->cov));
        }
        if (!n) { unset = true; return false; }
        const auto result = std::minmax_element(covs.begin(), covs.end());
        lowest = nd.contigs[inds[result.first - covs.begin()]];
        highest = nd.contigs[inds[result.second - covs.begin()]];
        return true;
    }

    // ---- removeChimerasAndClean: FGPU_PLAN_OK or FGPU_PLAN_UNSET; the graph knows its coverages (of_build with summaries, or set_cov);
    // inf.print is not touched
    int remove_chimeras_and_clean(fgpu_chimera_info& inf) {
        const uint64_t insert_size = 150;                            // removeChimericExtensions(150)
        if (!have_cov) return FGPU_PLAN_INPUT;
        inf.nodes_before = g.node_map.size();
        for (auto it = g.node_map.begin(); it != g.node_map.end();) {          // removeChimericExtensions
            const uint64_t node = it->first;
            Node& nd = it->second;
            bool erase = false;
            if (paths_out(nd) > 1) {
                int64_t P = NONE, Q = NONE, P2 = NONE, Q2 = NONE;
                if (!min_max_coverage(nd, P, Q)) return FGPU_PLAN_UNSET;
                const End far = other_end(tigs[P], node);
                if (!far.has || far.key == node) { inf.skipped[FGPU_CHIMERA_SKIP_NO_FAR]++; ++it; continue; }
                Node* far_node = node_at(far.key);
                if (!far_node) return FGPU_PLAN_UNSET;
                const int far_index = index_of(*far_node, P);
                if (far_index < 0) return FGPU_PLAN_UNSET;
                if (far_index == 4) { inf.skipped[FGPU_CHIMERA_SKIP_BACK]++; ++it; continue; }
                if (paths_out(*far_node) < 2) { inf.skipped[FGPU_CHIMERA_SKIP_FAR_PATHS]++; ++it; continue; }
                if (!min_max_coverage(*far_node, P2, Q2)) return FGPU_PLAN_UNSET;
                const double q = fgpu_cov_average(tigs[Q].cov), p = fgpu_cov_average(tigs[P].cov);
                const double q2 = fgpu_cov_average(tigs[Q2].cov), p2 = fgpu_cov_average(tigs[P2].cov);
                const double ratio1 = q / p;
                const double ratio2 = q2 / p2;
                if (tigs[P].len < insert_size && ratio1 >= 3 && P == P2) {
                    const int near_index = index_of(nd, P);
                    if (near_index < 0) return FGPU_PLAN_UNSET;
                    if (ratio1 > ratio2) {
                        cut_path(node, nd, near_index);
                        inf.cut_near++;
                    } else if (ratio2 > ratio1) {
                        cut_path(far.key, *far_node, far_index);
                        inf.cut_far++;
                    } else {
                        cut_path(node, nd, near_index);
                        const int again = index_of(*far_node, P);
                        if (again < 0) return FGPU_PLAN_UNSET;
                        cut_path(far.key, *far_node, again);
                        delete_contig(P);
                        inf.cut_both++;
                    }
                    if (unset) return FGPU_PLAN_UNSET;
                    if (is_collapsible(nd)) {
                        collapse_node(node, nd);
                        inf.collapsed[0]++;
                        inf.collapsed_after_cut++;
                        erase = true;
                    }
                    inf.removed++;
                } else {
                    inf.skipped[!(tigs[P].len < insert_size) ? FGPU_CHIMERA_SKIP_LONG : !(ratio1 >= 3) ? FGPU_CHIMERA_SKIP_RATIO : FGPU_CHIMERA_SKIP_OTHER_P]++;
                }
            } else if (is_collapsible(nd)) {
                collapse_node(node, nd);
                inf.collapsed[0]++;
                erase = true;
            }
            if (unset) return FGPU_PLAN_UNSET;
            if (erase) it = g.node_map.erase(it); else ++it;
        }
        inf.changed = inf.removed > 0;
        if (inf.changed) {
            inf.validated = 1;
            return validate_none_collapsible(inf.collapsed[1], inf.degenerate[1]);
        }
        return FGPU_PLAN_OK;
    }

    // ---- printContigs' two passes over the graph as it stands, into out's print arrays (n_print, n_print_pieces are set whatever the
    // room); the marks are the passes' own, so the graph is not changed.  FGPU_PLAN_OK, FGPU_PLAN_UNSET or FGPU_PLAN_SHORT
    int print_records(fgpu_tips_out* out, fgpu_raw_info& pr) {
        Room<uint64_t> print_first(out->print_first, out->print_first ? out->print_cap + 1 : 0);
        Room<uint32_t> print_number(out->print_number, out->print_cap);
        Room<fgpu_join_piece> print_pieces(out->print_pieces, out->print_pieces_cap);
        std::vector<char> mark(tigs.size(), 0);
        auto print = [&](const std::vector<fgpu_join_piece>& a, const std::vector<fgpu_join_piece>* b) {
            print_first.put(print_pieces.n);
            print_number.put((uint32_t)(print_number.n + 1));
            for (const auto& p : a) print_pieces.put(p);
            if (b) for (const auto& p : *b) print_pieces.put(p);
        };
        memset(&pr, 0, sizeof(pr));
        pr.nodes = g.node_map.size();
        for (auto& kv : g.node_map) {                                    // printAndMarkBubbleContigs
            const uint64_t node = kv.first;
            Node& nd = kv.second;
            if (paths_out(nd) != 2) continue;                            // isBubbleNode
            bool first_far = true, same = true;
            End far0 = {false, 0};
            for (int i = 0; i < 4; i++) {
                if (!(nd.cov[i] > 0)) continue;
                const Tig* t = tig_at(nd.contigs[i]);
                if (!t) return FGPU_PLAN_UNSET;                          // tig->otherEndNode(node) on a null tig
                const End far = other_end(*t, node);
                if (first_far) { far0 = far; first_far = false; }
                else same = far.has == far0.has && (!far.has || far.key == far0.key);
            }
            if (!same || !far0.has) continue;                            // allSame (:153-162): two null nodes are not the same
            if (!tig_at(nd.contigs[4])) return FGPU_PLAN_UNSET;          // back->getSeq() on a null back
            const int64_t back = nd.contigs[4];
            if (!(tigs[back].len < 250)) continue;
            bool back_mark = false;
            for (int i = 0; i < 4; i++) {
                const int64_t c = nd.contigs[i];
                if (c == NONE) continue;
                if (!tig_at(c)) return FGPU_PLAN_UNSET;
                if (mark[c]) continue;
                if (!mark[back]) {
                    Tig left = tigs[back], right = tigs[c];
                    if (side(left, node) == 1) reverse(left);
                    if (side(right, node) == 2) reverse(right);
                    print(left.list, &right.list);
                    pr.bubble_records++;
                    back_mark = true;
                    mark[c] = 1;
                }
            }
            if (back_mark) mark[back] = 1;
        }
        for (auto& kv : g.node_map) {                                    // printUnmarkedUnitigs
            Node& nd = kv.second;
            for (int i = 0; i < 5; i++) {
                const int64_t c = nd.contigs[i];
                if (c == NONE) continue;
                if (!tig_at(c)) return FGPU_PLAN_UNSET;
                if (mark[c]) continue;
                print(tigs[c].list, nullptr);
                pr.node_contigs++;
                mark[c] = 1;
            }
        }
        for (int64_t c : isolated) {
            if (tigs[c].len >= (uint64_t)(int64_t)read_length) {         // (size_t >= int: the int goes to unsigned)
                print(tigs[c].list, nullptr);
                pr.isolated_kept++;
            } else {
                pr.isolated_dropped++;
            }
        }
        print_first.put(print_pieces.n);
        pr.records = print_number.n;
        out->n_print = print_number.n; out->n_print_pieces = print_pieces.n;
        const bool fits = (!print_number.n || (print_number.n <= print_number.cap && print_first.n <= print_first.cap)) && print_pieces.fits();
        return fits ? FGPU_PLAN_OK : FGPU_PLAN_SHORT;
    }

    // ---- printGraph's walk over the graph as it stands (ContigIterator, then isolated_contigs): the FASTG records in file order.  Reads only:
    // the graph is not changed, not even its `unset` mark.  FGPU_PLAN_OK; FGPU_PLAN_UNSET wherever the reference would go through a pointer that is
    // null or gone, or asks Contig::getSide(node, index) for an end the contig does not have; FGPU_PLAN_INPUT: the graph knows no coverages, or
    // a neighbour is a contig the walk prints nowhere (its first end's slot does not hold it: no step leaves such a graph; the reference would
    // print its name, this plan has no record to name) -- FGPU_PLAN_UNSET comes first where the graph holds both
    int fastg_records(FastgPlan& out) const {
        out = FastgPlan();
        if (!have_cov) return FGPU_PLAN_INPUT;
        std::vector<int64_t> record_of(tigs.size(), NONE);
        auto live = [&](int64_t c) { return c != NONE && tigs[c].alive; };
        auto record = [&](int64_t c) {
            if (record_of[c] == NONE) record_of[c] = (int64_t)out.tig.size();
            out.tig.push_back(c);
        };
        for (const auto& kv : g.node_map) {                              // ContigIterator::findNextContig
            const uint64_t node = kv.first;
            for (int index = 0; index < 5; index++) {
                const int64_t c = kv.second.contigs[index];
                if (c == NONE) continue;
                if (!live(c)) return FGPU_PLAN_UNSET;
                const Tig& t = tigs[c];
                if (!t.has1 || !t.has2) { record(c); continue; }         // one side is a sink: always
                if (t.node1 == t.node2) {                                // both ends on one node: at the lower index
                    if (index == std::min(t.ind1, t.ind2)) record(c);
                    continue;
                }
                const int s = side_at(t, node, index);
                if (s < 0) return FGPU_PLAN_UNSET;
                if (s == 1) record(c);
            }
        }
        out.info.node_records = out.tig.size();
        out.info.nodes = g.node_map.size();
        out.info.isolated_listed = isolated.size();
        for (int64_t c : isolated) {
            if (!live(c)) return FGPU_PLAN_UNSET;
            if (tigs[c].len >= (uint64_t)(int64_t)read_length) {         // (size_t >= int: the int goes to unsigned)
                record(c);
                out.info.isolated_printed++;
            }
        }
        // Contig::getNeighbors: the primed header's (RC) through node1_p and ind1, the other's through node2_p and ind2
        int status = FGPU_PLAN_OK;
        bool nowhere = false;
        auto neighbours = [&](bool has, uint64_t key, int ind) {
            if (has) {
                const auto at = g.node_map.find(key);
                if (at == g.node_map.end()) { status = FGPU_PLAN_UNSET; return; }
                const Node& nd = at->second;
                for (int i = ind == 4 ? 0 : 4; i < (ind == 4 ? 4 : 5); i++) {          // ContigNode::getFastGNeighbors
                    const int64_t c = nd.contigs[i];
                    if (c == NONE) continue;
                    if (!live(c)) { status = FGPU_PLAN_UNSET; return; }
                    const int s = side_at(tigs[c], key, i);
                    if (s < 0) { status = FGPU_PLAN_UNSET; return; }
                    if (record_of[c] == NONE) { nowhere = true; continue; }     // (what is undefined elsewhere in the graph comes first: the walk goes on)
                    out.nbr.push_back((uint32_t)record_of[c] | (s == 2 ? FGPU_FASTG_PRIMED : 0u));
                }
            }
        };
        if (out.tig.size() >= (uint64_t)FGPU_FASTG_PRIMED) return FGPU_PLAN_INPUT;
        out.nbr_first.push_back(0);
        for (int64_t c : out.tig) {
            const Tig& t = tigs[c];
            neighbours(t.has1, t.node1, t.ind1);
            out.nbr_first.push_back(out.nbr.size());
            neighbours(t.has2, t.node2, t.ind2);
            out.nbr_first.push_back(out.nbr.size());
            if (status != FGPU_PLAN_OK) return status;
        }
        return nowhere ? FGPU_PLAN_INPUT : FGPU_PLAN_OK;
    }

    // ---- the graph as it stands, into out's nodes, contigs, list_first and pieces (n_nodes, n_contigs, n_pieces are set whatever the room).
    // FGPU_PLAN_OK or FGPU_PLAN_SHORT
    int graph_records(fgpu_tips_out* out) const {
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
        for (int64_t c : isolated) record(c, true);
        list_first.put(pieces.n);
        out->n_nodes = nodes.n; out->n_contigs = recs_out.n; out->n_pieces = pieces.n;
        const bool fits = nodes.fits() && (!recs_out.n || (recs_out.n <= recs_out.cap && list_first.n <= list_first.cap)) && pieces.fits();
        return fits ? FGPU_PLAN_OK : FGPU_PLAN_SHORT;
    }
};

}  // namespace fgpu_graph
#endif
