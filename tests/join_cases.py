"""Hand-made contigs and piece lists for the join (tests/detip_ref.py, fgpu_stage3_join): made once per k from a seed, shared by the CPU and
the GPU tests, left unchanged.  Every list is cut out of a master string -- consecutive pieces overlap by k bases, as the pieces of a
collapsed node's contigs do -- and some pieces are then stored reverse-complemented and flagged: the joined sequence must be the master."""
import functools

import numpy as np

from tests import contig_ref as R


def _random(rng, n):
    return "".join("ACGT"[i] for i in rng.integers(0, 4, size=n))


class Cases:
    def __init__(self, k, seed):
        self.k, self.rng = k, np.random.default_rng(seed)
        self.contigs, self.lists, self.masters, self.names = [], [], [], []

    def add(self, name, own, last, flips, n_cov=None, n_dist=None):
        """own: the bases every piece but the last gives (its length is own + k); last: the last piece's length; flips: one per piece"""
        k, rng = self.k, self.rng
        assert len(flips) == len(own) + 1 and last >= 1 and (last >= k or not own)
        master = _random(rng, sum(own) + last)
        pieces, at = [], 0
        for i, fl in enumerate(flips):
            n = own[i] + k if i < len(own) else last
            s = master[at:at + n]
            at += own[i] if i < len(own) else 0
            nc = n_cov[i] if n_cov else int(rng.integers(1, 5))
            nd = n_dist[i] if n_dist else int(rng.integers(0, 5))
            d, c = [int(v) for v in rng.integers(1, 256, size=nd)], [int(v) for v in rng.integers(0, 256, size=nc)]
            if fl:                                                             # stored as the other strand reads it; the flip reads it back
                s, d, c = R.revcomp_string(s), d[::-1], c[::-1]
            pieces.append((len(self.contigs), bool(fl)))
            self.contigs.append((s, d, c))
        self.lists.append(pieces)
        self.masters.append(master)
        self.names.append(name)


@functools.lru_cache(maxsize=None)
def cases(k):
    t = Cases(k, 1000 + k)
    t.add("single", [], 50, [0])
    t.add("single_flipped", [], 77, [1])
    t.add("single_shorter_than_k", [], 3, [1])                                # (only a joined piece needs k bases)
    t.add("two", [40], k + 9, [0, 0])
    t.add("two_flip_first", [40], k + 9, [1, 0])
    t.add("two_flip_second", [40], k + 9, [0, 1])
    t.add("five_mixed", [17, 70, 1, 33], k + 5, [0, 1, 1, 0, 1])
    t.add("middle_of_k_bases", [20, 0, 45], k + 2, [0, 1, 0, 0])              # a middle piece that gives no bases of its own
    t.add("first_of_k_bases", [0, 12], k, [1, 0, 1])
    t.add("all_of_k_bases", [0, 0, 0], k, [0, 1, 0, 1])
    t.add("run_of_4", [10, 5, 6], k + 3, [0, 0, 1, 0], n_cov=[3, 1, 1, 2])    # two middle pieces of one coverage entry each: a minimum over 4
    t.add("run_of_5_flipped", [10, 5, 6, 2], k + 3, [1, 1, 0, 1, 0], n_cov=[2, 1, 1, 1, 3])
    t.add("all_single_coverages", [4, 4, 4], k, [0, 1, 0, 1], n_cov=[1, 1, 1, 1])
    t.add("two_single_coverages", [9], k, [0, 0], n_cov=[1, 1])
    t.add("no_distances", [9, 9], k, [0, 1, 0], n_dist=[0, 0, 0])
    t.add("distances_only_in_the_middle", [9, 9], k, [1, 1, 1], n_dist=[0, 4, 0])
    for total in (31, 32, 33, 63, 64, 65):                                     # joined lengths around one word and two
        if total >= k:
            t.add("len%d_one" % total, [], total, [total & 1])
            t.add("len%d_three" % total, [total - k, 0], k, [0, 1, 1])
        if total - k >= 3:
            t.add("len%d_two" % total, [3], total - 3, [1, 0])
    t.add("starts_at_a_word", [32, 7], k + 1, [0, 1, 0])                       # the second piece's first own base is base 32
    t.add("starts_at_a_word_flipped_first", [64, 7], k + 1, [1, 0, 0])
    t.add("ends_on_a_word", [5, 27, 40], k, [1, 0, 1, 0])                      # the second piece's last own base is base 31
    t.add("long_pieces", [700, 1, 333], 500, [1, 0, 1, 1], n_cov=[90, 1, 70, 130], n_dist=[89, 0, 69, 129])   # lists longer than a wave
    rng = np.random.default_rng(2000 + k)
    for i in range(150):                                                       # every seam offset, piece count and flip pattern a few times over
        m = int(rng.integers(1, 9))
        t.add("random%d" % i, [int(v) for v in rng.integers(0, 71, size=m - 1)], k + int(rng.integers(0, 71)), [int(v) for v in rng.integers(0, 2, size=m)])
    return t
