"""An independent reference for the dump order of the junctions: the node list of libstdc++'s std::unordered_map, replayed link by link.

The container keeps ALL its nodes on one singly linked list and a bucket points at the node BEFORE its first node
(bits/hashtable.h).  Two rules move nodes:

  * a node inserted into an empty bucket goes to the head of the whole list; into a non-empty bucket it goes right behind that
    bucket's "before" node (_M_insert_bucket_begin);
  * a rehash walks the list as it stands and re-inserts every node by the same two rules into the new buckets (_M_rehash_aux,
    unique keys).

`replay` does exactly that on flat index lists, for ANY schedule of rehashes -- several at one count, shrinking bucket counts, a
rehash after the last insertion.  It is deliberately NOT the sort-based closed form of faucet_amd/host/junction_order.h: the
closed form is what the device computes (fgpu_scan_dump_order), and this is what it is compared with.  The hash of a 64-bit key is
the key.  tests/test_dump_order_ref_cpu.py pins `replay` and `LIBSTDCXX_SCHEDULE` to a real container.
"""
import numpy as np

_NIL = -1    # no node
_HEAD = -2   # the list's before-begin sentinel in the role of a bucket's "before" node

# WHEN libstdc++'s container rehashes while keys are inserted one by one, and to how many buckets: (nodes present, buckets from then
# on), the first entry being the empty container's.  What DumpOrder::schedule(300000) gives (std::__detail::_Prime_rehash_policy).
LIBSTDCXX_SCHEDULE = ((0, 1), (0, 13), (13, 29), (29, 59), (59, 127), (127, 257), (257, 541), (541, 1109), (1109, 2357), (2357, 5087),
                      (5087, 10273), (10273, 20753), (20753, 42043), (42043, 85229), (85229, 172933), (172933, 351061))


def libstdcxx_schedule(n):
    """(counts, buckets) of the library's schedule for n keys: the entries whose count is below n, and always (0, 1) and (0, 13)"""
    if n > LIBSTDCXX_SCHEDULE[-1][1]:
        raise ValueError("LIBSTDCXX_SCHEDULE ends at %d keys" % LIBSTDCXX_SCHEDULE[-1][1])
    sch = [e for i, e in enumerate(LIBSTDCXX_SCHEDULE) if i < 2 or e[0] < n]
    return [c for c, _ in sch], [b for _, b in sch]


def crowded_k5_sets():
    """k = 5: every key below 1024, so the buckets are crowded whatever their number (the sets of tests/host/junction_order_check.cpp: 700
    keys by the strides 389 and 7919, ascending, and all 1024 keys descending -- and all 1024 ascending)"""
    i = np.arange(1024, dtype=np.uint64)
    return {"stride389": (i[:700] * np.uint64(389)) % np.uint64(1024), "stride7919": (i[:700] * np.uint64(7919)) % np.uint64(1024),
            "ascending": i[:700].copy(), "descending_all": np.uint64(1023) - i, "ascending_all": i.copy()}


def replay(keys, counts, buckets, n=None):
    """The container's iteration order, as indices into keys[:n] (uint32), after inserting keys[0], keys[1], ... keys[n - 1] into a
    container that goes to buckets[j] buckets when counts[j] nodes are present (a rehash at count n comes after the last insertion).
    Keys must be distinct."""
    keys = [int(x) for x in (keys.tolist() if isinstance(keys, np.ndarray) else keys)]
    n = len(keys) if n is None else int(n)
    counts, buckets = [int(c) for c in counts], [int(b) for b in buckets]
    if len(counts) != len(buckets) or not counts or counts[0] != 0:
        raise ValueError("a schedule starts with (0, buckets of the empty container)")
    if any(a > b for a, b in zip(counts, counts[1:])) or counts[-1] > n or min(buckets) < 1 or n > len(keys):
        raise ValueError("counts must not descend nor exceed n, bucket counts must be positive")
    nxt = [_NIL] * n       # the list
    head = _NIL
    before = {}            # bucket -> the node before its first node (only non-empty buckets are present)
    n_buckets = None
    at = 0                 # next entry of the schedule
    for i in range(n + 1):
        while at < len(counts) and counts[at] == i:
            # rehash: relink the nodes in list order
            n_buckets = buckets[at]
            at += 1
            before = {}
            p, head = head, _NIL
            begin_bucket = 0
            while p != _NIL:
                following = nxt[p]
                b = keys[p] % n_buckets
                q = before.get(b, _NIL)
                if q == _NIL:
                    nxt[p] = head
                    head = p
                    before[b] = _HEAD
                    if nxt[p] != _NIL:
                        before[begin_bucket] = p
                    begin_bucket = b
                elif q == _HEAD:
                    nxt[p] = head
                    head = p
                else:
                    nxt[p] = nxt[q]
                    nxt[q] = p
                p = following
        if i == n:
            break
        b = keys[i] % n_buckets
        q = before.get(b, _NIL)
        if q == _NIL:
            nxt[i] = head
            head = i
            if nxt[i] != _NIL:
                before[keys[nxt[i]] % n_buckets] = i
            before[b] = _HEAD
        elif q == _HEAD:
            nxt[i] = head
            head = i
        else:
            nxt[i] = nxt[q]
            nxt[q] = i
    order = np.empty(n, dtype=np.uint32)
    p, j = head, 0
    while p != _NIL:
        order[j] = p
        j += 1
        p = nxt[p]
    assert j == n, "repeated keys, or a broken list"
    return order
