// host_detip.cpp — the host route of scripts/stage3_detip_times.py: the FASTA of fgpu_tips_plan's print records (piece lists over the contigs of a
// build) joined and printed on the HOST from the 2-bit words fgpu_stage3_build_take hands over, one thread, base by base -- what a caller would do
// without fgpu_stage3_join and fgpu_stage3_fasta_joined.  Measurement only: the script compiles it into a temporary shared object; nothing of the
// product links it.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../include/faucet_gpu.h"

static void piece(std::string& s, const uint64_t* text, const fgpu_contig& c, bool flip, size_t drop) {
    static const char fwd[4] = {'A', 'C', 'T', 'G'}, rev[4] = {'T', 'G', 'A', 'C'};
    const uint64_t* w = text + c.text_word;
    const size_t n = c.len - drop;
    if (!flip) for (size_t i = 0; i < n; i++) s.push_back(fwd[(w[i >> 5] >> (2 * (i & 31))) & 3]);
    else for (size_t i = 0; i < n; i++) { const size_t j = c.len - 1 - i; s.push_back(rev[(w[j >> 5] >> (2 * (j & 31))) & 3]); }
}

// returns the bytes written (out may be null: count only)
extern "C" uint64_t host_detip_fasta(const uint64_t* first, const uint32_t* number, uint64_t n, const fgpu_join_piece* pieces, const fgpu_contig* contigs,
                                     const uint64_t* text, int32_t k, char* out) {
    uint64_t at = 0;
    std::string s, rc;
    char head[32];
    for (uint64_t i = 0; i < n; i++) {
        s.clear();
        for (uint64_t p = first[i]; p < first[i + 1]; p++) piece(s, text, contigs[pieces[p].call], pieces[p].flip != 0, p + 1 < first[i + 1] ? (size_t)k : 0);
        rc.resize(s.size());
        for (size_t j = 0; j < s.size(); j++) { const char c = s[s.size() - 1 - j]; rc[j] = c == 'A' ? 'T' : c == 'C' ? 'G' : c == 'G' ? 'C' : 'A'; }
        const std::string& keep = s <= rc ? s : rc;
        const int h = snprintf(head, sizeof(head), ">Contig%u\n", number[i]);
        if (out) { memcpy(out + at, head, h); memcpy(out + at + h, keep.data(), keep.size()); out[at + h + keep.size()] = '\n'; }
        at += h + keep.size() + 1;
    }
    return at;
}
