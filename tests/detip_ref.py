"""Contigs that are joins of contigs, restated in plain Python: what fgpu_stage3_join (faucet_amd/csrc/stage3_join.hip) computes on the device.

A contig is (sequence, distances, coverages), the three members of the reference's ContigJuncList; a piece is (contig, flip).

  join(contigs, lists, k)        the reference's own steps, one after the other: ContigJuncList::reverse (utils/ContigJuncList.cpp:98-103) on
                                 every flipped piece, then ContigJuncList::concatenate (:107-123) left to right, as Contig::concatenate
                                 (src/Contig.cpp:83-109) calls them.  tests/golden/join_concat.json.gz holds what the compiled reference
                                 makes of the same lists (tests/golden/make_join_golden.py).
  join_by_entry(...)             the same results found entry by entry, the way the kernels find them -- three running sums per piece, then every
                                 word of text, every distance and every coverage on its own from a search over those sums -- in Python
                                 integers: the index arithmetic of the kernels, checked without a device against join().
  pack(contigs)                  the contigs as the library lays them out (fgpu_stage3_contigs_take's arrays and an fgpu_contig per contig)
"""
import bisect

from tests import contig_ref as R


def oriented(contig, flip):
    """ContigJuncList::reverse: both lists reversed, the sequence reverse-complemented"""
    s, d, c = contig
    return (R.revcomp_string(s), list(d)[::-1], list(c)[::-1]) if flip else (s, list(d), list(c))


def concatenate(a, b, k):
    """ContigJuncList::concatenate (utils/ContigJuncList.cpp:107-123)"""
    cov = a[2][:-1] + [min(a[2][-1], b[2][0])] + b[2][1:]
    return a[0][:len(a[0]) - k] + b[0], a[1] + b[1], cov


def join(contigs, lists, k):
    """per list of (contig index, flip): (sequence, distances, coverages, getAvgCoverage())"""
    out = []
    for pieces in lists:
        acc = oriented(contigs[pieces[0][0]], pieces[0][1])
        for c, flip in pieces[1:]:
            acc = concatenate(acc, oriented(contigs[c], flip), k)
        total = 0.0
        for v in acc[2]:                                                       # (ContigJuncList::getAvgCoverage :166-176: a double, entry by entry)
            total += float(v)
        out.append((acc[0], acc[1], acc[2], total / len(acc[2])))
    return out


def reverse_list(pieces):
    """the piece list of the reversed contig: the list reversed, every flip toggled"""
    return [(c, not flip) for c, flip in reversed(pieces)]


def pack(contigs):
    """(CONTIG_DTYPE array, text words, distances, coverages): every string from a word of its own, A 0, C 1, T 2, G 3, first base lowest"""
    import numpy as np
    from faucet_amd import api
    rec = np.zeros(len(contigs), dtype=api.CONTIG_DTYPE)
    words, dist, cov = [], [], []
    for i, (s, d, c) in enumerate(contigs):
        rec[i]["text_word"], rec[i]["seg_first"], rec[i]["cov_first"] = len(words), len(dist), len(cov)
        rec[i]["len"], rec[i]["n_seg"], rec[i]["n_cov"] = len(s), len(d), len(c)
        for at in range(0, len(s), 32):
            words.append(sum(R.NT.index(ch) << (2 * j) for j, ch in enumerate(s[at:at + 32])))
        dist += list(d)
        cov += list(c)
    return rec, np.array(words, dtype=np.uint64), np.array(dist, dtype=np.uint8), np.array(cov, dtype=np.uint8)


def _window(word_list, length, a):
    """bases a .. a + 31 of a 2-bit string as one 64-bit value, base a lowest; fields outside the string are 0 here"""
    v = 0
    for j in range(32):
        if 0 <= a + j < length:
            v |= ((word_list[(a + j) >> 5] >> (2 * ((a + j) & 31))) & 3) << (2 * j)
    return v


def _revcomp32(x):
    r = 0
    for j in range(32):
        r |= (((x >> (2 * j)) & 3) ^ 2) << (2 * (31 - j))
    return r


def join_by_entry(contigs, lists, k):
    """join()'s results, each output element computed on its own as the kernels compute it"""
    words_of = [[sum(R.NT.index(ch) << (2 * j) for j, ch in enumerate(s[at:at + 32])) for at in range(0, len(s), 32)] for s, _, _ in contigs]
    flat = [pc for pl in lists for pc in pl]
    first = [0]
    for pl in lists:
        first.append(first[-1] + len(pl))
    base, dist, cov = [0], [0], [0]
    for i, pl in enumerate(lists):
        for j, (c, _) in enumerate(pl):
            last = j + 1 == len(pl)
            s, d, v = contigs[c]
            base.append(base[-1] + (len(s) if last else len(s) - k))
            dist.append(dist[-1] + len(d))
            cov.append(cov[-1] + (len(v) if last else len(v) - 1))
    out = []
    for i in range(len(lists)):
        p0, p1 = first[i], first[i + 1]
        length = base[p1] - base[p0]
        text = []
        for g in range((length + 31) // 32):                                   # k_join_text: one word
            at, end = base[p0] + 32 * g, base[p1]
            p = bisect.bisect_right(base, at, p0, p1 + 1) - 1
            w = fill = 0
            while fill < 32 and at + fill < end:
                c, flip = flat[p]
                own, off = base[p + 1] - base[p], at + fill - base[p]
                if off < own:
                    take = min(own - off, 32 - fill)
                    n = len(contigs[c][0])
                    win = _revcomp32(_window(words_of[c], n, n - 32 - off)) if flip else _window(words_of[c], n, off)
                    w |= (win & ((1 << (2 * take)) - 1)) << (2 * fill)
                    fill += take
                p += 1
            text.append(w)
        seq = "".join(R.NT[(text[b >> 5] >> (2 * (b & 31))) & 3] for b in range(length))
        assert not text or text[-1] >> (2 * ((length - 1) % 32 + 1)) == 0      # the bits behind the last base
        ds = []
        for e in range(dist[p0], dist[p1]):                                    # k_join_dist: one distance
            p = bisect.bisect_right(dist, e, 0, len(flat) + 1) - 1
            c, flip = flat[p]
            d = contigs[c][1]
            ds.append(d[len(d) - 1 - (e - dist[p])] if flip else d[e - dist[p]])
        cs = []
        for j in range(cov[p0], cov[p1]):                                      # k_join_cov: one coverage
            p = bisect.bisect_right(cov, j, p0, p1 + 1) - 1
            v = 255
            while True:
                c, flip = flat[p]
                x = contigs[c][2]
                o = j - cov[p]
                if o >= len(x):
                    break
                v = min(v, x[len(x) - 1 - o] if flip else x[o])
                if p == p0:
                    break
                p -= 1
            cs.append(v)
        out.append((seq, ds, cs, float(sum(cs)) / len(cs)))
    return out
