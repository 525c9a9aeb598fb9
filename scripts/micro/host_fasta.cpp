// host_fasta.cpp — the baseline of scripts/stage3_raw_contigs_times.py: the FASTA of fgpu_fasta_seq records assembled on the HOST from the
// 2-bit words fgpu_stage3_build_take hands over, one thread, base by base -- what a caller had to do before fgpu_stage3_fasta.  Measurement
// only: the script compiles it into a temporary shared object; nothing of the product links it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/faucet_gpu.h"

static void piece(std::string& s, const uint64_t* text, const fgpu_fasta_seq& q, int p, size_t drop) {
    static const char fwd[4] = {'A', 'C', 'T', 'G'}, rev[4] = {'T', 'G', 'A', 'C'};
    const uint64_t* w = text + q.text_word[p];
    const size_t n = q.len[p] - drop;
    if (!q.flip[p]) for (size_t i = 0; i < n; i++) s.push_back(fwd[(w[i >> 5] >> (2 * (i & 31))) & 3]);
    else for (size_t i = 0; i < n; i++) { const size_t j = q.len[p] - 1 - i; s.push_back(rev[(w[j >> 5] >> (2 * (j & 31))) & 3]); }
}

// returns the bytes written (out may be null: count only)
extern "C" uint64_t host_fasta(const fgpu_fasta_seq* seqs, uint64_t n, const uint64_t* text, int32_t k, char* out) {
    uint64_t at = 0;
    std::string s, rc;
    char head[32];
    for (uint64_t i = 0; i < n; i++) {
        const fgpu_fasta_seq& q = seqs[i];
        s.clear();
        piece(s, text, q, 0, q.pieces == 2 ? (size_t)k : 0);
        if (q.pieces == 2) piece(s, text, q, 1, 0);
        rc.resize(s.size());
        for (size_t j = 0; j < s.size(); j++) { const char c = s[s.size() - 1 - j]; rc[j] = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }
        const std::string& keep = s <= rc ? s : rc;
        const int h = snprintf(head, sizeof(head), ">Contig%u\n", q.number);
        if (out) { memcpy(out + at, head, h); memcpy(out + at + h, keep.data(), keep.size()); out[at + h + keep.size()] = '\n'; }
        at += h + keep.size() + 1;
    }
    return at;
}
