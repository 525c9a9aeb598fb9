// host_fastg.cpp — the yardstick of scripts/stage3_fastg_times.py: ContigGraph::printGraph's file made ON THE HOST, one thread, from what exists
// without fgpu_stage3_graph_fastg -- the graph fgpu_stage3_graph_take hands out (nodes, contig records) and its contigs joined by fgpu_stage3_join and
// taken to the host (fgpu_joined records, 2-bit text).  The walk is ContigIterator's, the names fastg_name.h's; <this> is the contig's record number.
// MEASUREMENT ONLY.  out == NULL: the size alone.
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

#include "../../faucet_amd/csrc/fastg_name.h"
#include "../../include/faucet_gpu.h"

namespace {
struct Name { char s[FGPU_FASTG_NAME_STRIDE]; uint32_t len; };
struct Out {
    char* p;
    uint64_t n = 0;
    void put(const char* s, uint64_t len) { if (p) memcpy(p + n, s, len); n += len; }
    void put(char c) { if (p) p[n] = c; n++; }
};
int side_at(const fgpu_tips_contig& t, uint64_t node, int index) {
    if (t.has1 && t.node1 == node && t.ind1 == index) return 1;
    if (t.has2 && t.node2 == node && t.ind2 == index) return 2;
    return -1;
}
}  // namespace

extern "C" uint64_t host_fastg(const fgpu_tips_node* nodes, uint64_t n_nodes, const fgpu_tips_contig* contigs, uint64_t n_contigs, const fgpu_joined* joined,
                               const uint64_t* text, int32_t read_length, char* out_bytes) {
    std::vector<Name> names(n_contigs);
    for (uint64_t c = 0; c < n_contigs; c++) names[c].len = fgpu_fastg_name(c, joined[c].len, joined[c].cov_sum, joined[c].n_cov, names[c].s);
    std::unordered_map<uint64_t, uint64_t> at;
    at.reserve(n_nodes * 2);
    for (uint64_t i = 0; i < n_nodes; i++) at[nodes[i].key] = i;
    std::vector<uint64_t> records;
    for (uint64_t i = 0; i < n_nodes; i++)
        for (int index = 0; index < 5; index++) {
            const int32_t c = nodes[i].slot[index];
            if (c < 0) continue;
            const fgpu_tips_contig& t = contigs[c];
            if (!t.has1 || !t.has2) records.push_back(c);
            else if (t.node1 == t.node2) { if (index == (t.ind1 < t.ind2 ? t.ind1 : t.ind2)) records.push_back(c); }
            else if (side_at(t, nodes[i].key, index) == 1) records.push_back(c);
        }
    for (uint64_t c = 0; c < n_contigs; c++)
        if (contigs[c].isolated && joined[c].len >= (uint64_t)(int64_t)read_length) records.push_back(c);
    Out o{out_bytes};
    std::vector<char> seq;
    for (uint64_t c : records) {
        const fgpu_tips_contig& t = contigs[c];
        const uint32_t len = joined[c].len;
        const uint64_t* w = text + joined[c].text_word;
        seq.resize(len);
        for (uint32_t b = 0; b < len; b++) seq[b] = "ACTG"[(w[b >> 5] >> (2 * (b & 31))) & 3];
        for (int h = 0; h < 2; h++) {
            o.put('>');
            o.put(names[c].s, names[c].len);
            if (h == 0) o.put('\'');
            const bool has = h == 0 ? t.has1 : t.has2;
            const uint64_t key = h == 0 ? t.node1 : t.node2;
            const int ind = h == 0 ? t.ind1 : t.ind2;
            bool any = false;
            if (has) {
                const fgpu_tips_node& nd = nodes[at[key]];
                for (int i = ind == 4 ? 0 : 4; i < (ind == 4 ? 4 : 5); i++) {
                    const int32_t nb = nd.slot[i];
                    if (nb < 0) continue;
                    o.put(any ? ',' : ':');
                    any = true;
                    o.put(names[nb].s, names[nb].len);
                    if (side_at(contigs[nb], key, i) == 2) o.put('\'');
                }
            }
            o.put(';');
            o.put('\n');
            if (h == 0) {
                o.put(seq.data(), len);
            } else {
                if (o.p)
                    for (uint32_t b = 0; b < len; b++) {
                        const char x = seq[len - 1 - b];
                        o.p[o.n + b] = x == 'A' ? 'T' : x == 'C' ? 'G' : x == 'G' ? 'C' : 'A';
                    }
                o.n += len;
            }
            o.put('\n');
        }
    }
    return o.n;
}
