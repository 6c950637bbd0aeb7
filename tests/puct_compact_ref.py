"""Plain-numpy restatement of gz_selfplay_puct_compact (csrc/gz_puct_compact.hip): the
hole-filling plan and what it moves, on host copies of the slot buffer and of the
self-play workspace.  Layouts: SlotHeader (csrc/gz_search.h), PuctHdr and the tree
arrays (csrc/gz_puct.h), offsets from gz_selfplay_puct_layout."""
import numpy as np

PEND_SLOT_BYTES = 200 * 225 * 2  # uint16 [200][225] per slot
TREE_WIDTHS = (8, 1800, 4, 4, 64, 450, 2, 1, 1)  # W, prior, visits, value, board, child, parent, move, term
SLOT_GAME_ID, SLOT_N_MOVES, SLOT_GAME_ID_END = 64, 80, 88  # byte offsets in SlotHeader
TREE_N_NODES = 84  # byte offset in PuctHdr


def plan(active):
    """active: bool [n] -> (a, holes, fillers, order).  a = the active count; the holes
    are the idle slots below a, the fillers the active ones at or above a, both
    ascending; order[s] = the new index of old slot s: the identity except that the
    k-th filler and the k-th hole trade places."""
    active = np.asarray(active, bool)
    idx = np.arange(len(active))
    a = int(active.sum())
    holes = idx[~active & (idx < a)]
    fillers = idx[active & (idx >= a)]
    order = idx.copy()
    order[holes] = fillers
    order[fillers] = holes
    return a, holes, fillers, order


def slot_field(slots, offset, dtype):
    """One header field of every slot; slots: uint8 [n, slot_bytes]."""
    size = np.dtype(dtype).itemsize
    return np.ascontiguousarray(slots[:, offset:offset + size]).view(dtype)[:, 0]


def active_mask(slots):
    return slot_field(slots, SLOT_GAME_ID, np.int64) < slot_field(slots, SLOT_GAME_ID_END, np.int64)


def expected_slots(slots, n_active):
    """The slot buffer after a compaction of its first n_active slots."""
    _, holes, fillers, _ = plan(active_mask(slots[:n_active]))
    out = slots.copy()
    out[holes] = slots[fillers]
    out[fillers] = slots[holes]
    return out


def expected_workspace(ws, slots, n_active, layout, S, move_trees):
    """The self-play workspace (uint8 [bytes]) after a compaction: every filler's pending
    rows [0, n_moves) and, with move_trees, its tree header and rows [0, n_nodes) of each
    array at the hole's places; every other byte as it was."""
    pend0, _, tree0, stride = (int(x) for x in layout)
    M = S + 1
    _, holes, fillers, _ = plan(active_mask(slots[:n_active]))
    n_moves = slot_field(slots, SLOT_N_MOVES, np.int32)
    out = ws.copy()
    for h, f in zip(holes, fillers):
        nb = min(max(int(n_moves[f]), 0), 200) * 450
        src, dst = pend0 + int(f) * PEND_SLOT_BYTES, pend0 + int(h) * PEND_SLOT_BYTES
        out[dst:dst + nb] = ws[src:src + nb]
        if not move_trees:
            continue
        src, dst = tree0 + int(f) * stride, tree0 + int(h) * stride
        nn = min(max(int(ws[src + TREE_N_NODES:src + TREE_N_NODES + 4].view(np.int32)[0]), 0), M)
        out[dst:dst + 128] = ws[src:src + 128]
        off = 128
        for w in TREE_WIDTHS:
            out[dst + off:dst + off + w * nn] = ws[src + off:src + off + w * nn]
            off += w * M
    return out
