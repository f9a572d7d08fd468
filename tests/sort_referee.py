"""Exact referee of the in-tree radix sort (csrc/rsa_radix.hpp) and of classify_solo_kernel (csrc/rsa_sorted.hip): what the
sorted pairs, the solo flags, the flagged payloads and the owner side's query runs must be, bit for bit, from plain torch on the
CPU.  The sort is stable and its keys are integers, so there is one right answer and every comparison is ``torch.equal``.

A pair is one 8-byte word ``key << 32 | element``; keys are below 2^31, so the int64 view of a pair is non-negative and pairs
compare as the kernels' uint64 words do.  Everything here takes and returns CPU tensors."""
import torch

# ---- the host plan of rsa_radix.hpp, restated ONCE for the tests (test_sort_referee.py pins these formulas to the plans the GPU
# cases are named after: a change of RDX_SLOTS / RDX_ITEMS_MAX in the header moves those shapes knowingly)
RDX_TILE = 4096                # at most this many elements: radix_small_kernel (one workgroup, all passes in one launch)
RDX_DIGIT_BITS = 8
RDX_ITEMS_MIN, RDX_ITEMS_MAX = 4, 17
RDX_SLOTS = 1024
RDX_INLINE_SCAN_TILES = 8      # up to this many tiles the scatter pass sums the tile counts itself (no radix_scan_kernel)
SOLO_BIT = 1 << 31             # bit 31 of the payload: classify_solo_kernel's mark on a solo pair
SHARD_HDR = 2                  # RSA_SHARD_HDR: header words of a received segment (word 0 = the live count)
MOSTLY_SOLO_RATIO = 0.69       # classify_solo: total < 0.69 * rows -> flags preset to 1, zeros stored


def radix_items(total):
    """radix_items(): rows of 64 per wave of the multi-pass kernels (tile = 256 * items elements)"""
    round_cap = RDX_SLOTS * 256 * RDX_ITEMS_MAX
    rounds = 1 if total <= round_cap else -(-total // round_cap)
    per = rounds * RDX_SLOTS * 256
    return max(-(-total // per), RDX_ITEMS_MIN)


def radix_tiles(total):
    return -(-total // (256 * radix_items(total)))


def radix_key_bits(n_keys):
    """bits needed for keys 0 .. n_keys - 1 (at least 1, at most 32)"""
    b = 1
    while b < 32 and (1 << b) < n_keys:
        b += 1
    return b


def radix_passes(n_keys):
    return -(-radix_key_bits(n_keys) // RDX_DIGIT_BITS)


def plan(total):
    """('small',) for the one-workgroup sort, else ('multi', items, tiles, 'inline' | 'scan')"""
    if total <= RDX_TILE:
        return ('small',)
    tiles = radix_tiles(total)
    return ('multi', radix_items(total), tiles, 'inline' if tiles <= RDX_INLINE_SCAN_TILES else 'scan')


def mostly_solo(total, rows):
    """the polarity classify_solo picks"""
    return float(total) < MOSTLY_SOLO_RATIO * float(rows)


# ---- keys
def item_keys(ids, n_items):
    """SrcStepIds: a negative id is an empty slot (key n_items, behind every row), an id >= n_items is clamped to the last row"""
    ids = ids.to(torch.int64)
    return torch.where(ids < 0, torch.full_like(ids, n_items), ids.clamp(max=n_items - 1))


def step_ids(pos_ids, neg_ids):
    """[M * w] ids in element order e = m * w + c, c = 0 the positive when given"""
    neg_ids = neg_ids.reshape(neg_ids.shape[0], -1) if neg_ids.dim() > 1 else neg_ids.reshape(-1, 1)
    if pos_ids is None:
        return neg_ids.reshape(-1)
    return torch.cat([pos_ids.reshape(-1, 1), neg_ids.reshape(pos_ids.numel(), -1)], dim=1).reshape(-1)


def pairs_of_keys(keys):
    """the stable sort of (key, element) -> int64 pairs ``key << 32 | element``"""
    sk, order = torch.sort(keys.to(torch.int64), stable=True)
    return (sk << 32) | order


def pair_keys(pairs):
    return pairs >> 32


def pair_elems(pairs):
    """the element number: the payload without the solo mark"""
    return pairs & (SOLO_BIT - 1)


# ---- the sorts
def expected_step_pairs(pos_ids, neg_ids, n_items):
    """rsa_sort_step_elements / rsa_rows_update_sorted"""
    return pairs_of_keys(item_keys(step_ids(pos_ids, neg_ids), n_items))


def step_all_keys(pos_ids, neg_ids, user_ids, n_items, n_users):
    """SrcStepAll: the item elements, then element t_items + m with key n_items + 1 + user id (a negative user id sorts behind
    every real user, one >= n_users is clamped to the last)"""
    u = user_ids.to(torch.int64)
    u = torch.where(u < 0, torch.full_like(u, n_users), u.clamp(max=n_users - 1))
    return torch.cat([item_keys(step_ids(pos_ids, neg_ids), n_items), n_items + 1 + u])


def expected_step_all_pairs(pos_ids, neg_ids, user_ids, n_items, n_users):
    """rsa_bpr_sgd_prepare: [0, t_items) is the item part, the user part lies behind it"""
    return pairs_of_keys(step_all_keys(pos_ids, neg_ids, user_ids, n_items, n_users))


def segment_keys(keys, n_seg, stride, by_query, dead_key, extra_rows=None):
    """SrcSegments: element = slot number; header word 0 of a segment is its live count; the header slots and the slots outside
    the live range get ``dead_key``; a live slot's key is its query ((k >> 32) & 0x7fffffff) or its row (k & 0xffffffff), capped at
    ``dead_key``.  ``extra_rows`` (row sort only): the positives follow as elements slots + i, a negative row -> ``dead_key``."""
    k = keys.to(torch.int64).reshape(n_seg, stride)
    within = torch.arange(stride, dtype=torch.int64).unsqueeze(0)
    live = (within >= SHARD_HDR) & (within - SHARD_HDR < k[:, :1])
    key = ((k >> 32) & 0x7fffffff) if by_query else (k & 0xffffffff)
    out = torch.where(live, key.clamp(max=dead_key), torch.full_like(key, dead_key)).reshape(-1)
    if extra_rows is not None:
        r = extra_rows.to(torch.int64)
        out = torch.cat([out, torch.where(r < 0, torch.full_like(r, dead_key), (r & 0xffffffff).clamp(max=dead_key))])
    return out


def expected_segment_pairs(keys, n_seg, stride, by_query, dead_key, extra_rows=None):
    """the owner side's sorts by row (dead_key = n_rows, with the positives) and by query (dead_key = n_query_rows)"""
    return pairs_of_keys(segment_keys(keys, n_seg, stride, by_query, dead_key, extra_rows))


# ---- classification
def expected_solo(sorted_keys, pad_row, drop_key):
    """classify_solo_kernel, in SORTED order: position i is solo iff its key differs from both neighbours and is neither the
    padding row (``pad_row`` < 0: there is none) nor ``drop_key``"""
    k = sorted_keys.to(torch.int64)
    t = k.numel()
    solo = torch.ones(t, dtype=torch.bool)
    if t > 1:
        same = k[1:] == k[:-1]
        solo[1:] &= ~same
        solo[:-1] &= ~same
    solo &= k != drop_key
    if pad_row >= 0:
        solo &= k != pad_row
    return solo


def expected_flags(pairs, solo_sorted):
    """uint8 flags in ELEMENT order"""
    flags = torch.zeros(pairs.numel(), dtype=torch.uint8)
    flags[pair_elems(pairs)[solo_sorted]] = 1
    return flags


def expected_flagged_pairs(pairs, solo_sorted):
    """the pairs as the classification leaves them: bit 31 of the payload set exactly on the solo pairs"""
    return torch.where(solo_sorted, pairs | SOLO_BIT, pairs)


def expected_classified(pairs, pad_row, drop_key):
    """(flags in element order, flagged pairs) of a classification over all of ``pairs``"""
    solo = expected_solo(pair_keys(pairs), pad_row, drop_key)
    return expected_flags(pairs, solo), expected_flagged_pairs(pairs, solo)


# ---- the owner side's query runs
def expected_runs(q_pairs, n_queries):
    """query_runs_kernel: run_start[q] / run_end[q] (int32, 0 / 0 for a query without slots) over the query-sorted pairs"""
    k = pair_keys(q_pairs)
    t = k.numel()
    start = torch.zeros(n_queries, dtype=torch.int32)
    end = torch.zeros(n_queries, dtype=torch.int32)
    if t == 0:
        return start, end
    pos = torch.arange(t, dtype=torch.int64)
    first = torch.ones(t, dtype=torch.bool)
    first[1:] = k[1:] != k[:-1]
    last = torch.ones(t, dtype=torch.bool)
    last[:-1] = k[1:] != k[:-1]
    real = k < n_queries
    start[k[first & real]] = pos[first & real].to(torch.int32)
    end[k[last & real]] = (pos[last & real] + 1).to(torch.int32)
    return start, end
