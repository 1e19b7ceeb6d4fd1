"""TEST INFRASTRUCTURE: the gene-tree tests of checkm_amd/csrc/genetree_dev.h in numpy and plain Python, by other means than the header's:
class counts below a node come from one cumulative sum over a one-hot matrix of all classes of a rank, common ancestors from explicit
root paths, the conspecific test from Python sets.  The summation ORDER of a patristic distance is the header's (it is part of the
definition): up the first side, the second side added onto the same sum; two root distances, each from the leaf up and the root's own
length last, when the ancestor is the root.  genetree_check and genetree_run take the arguments of their namesakes in checkm_amd._lib
(ctx is ignored) and return the same.  Never imported by checkm_amd."""
import numpy as np

NONE = 0xffffffff
MAX_LEAVES, MAX_NODES, MAX_CLASSES = 1 << 14, 1 << 15, 65535


def _error(code, msg):
    from checkm_amd import _lib as real
    return real.CkmError(code, msg)


def genetree_check(t):
    """The size limits and the finite lengths; the structural tests of the header are the host executor's to make."""
    for k in range(t.ntrees):
        if t.leaf_off[k + 1] - t.leaf_off[k] > MAX_LEAVES or t.node_off[k + 1] - t.node_off[k] > MAX_NODES or \
                any(t.class_off[3 * k + r + 1] - t.class_off[3 * k + r] > MAX_CLASSES for r in range(3)):
            raise _error(-7, "tree %d is beyond a size limit" % k)
    if not np.isfinite(t.length).all():
        raise _error(-1, "an edge length is not finite")


def tree_bytes(t, k):
    g0, g1 = int(t.group_off[k]), int(t.group_off[k + 1])
    return (int(t.node_off[k + 1] - t.node_off[k]) * 21 + int(t.leaf_off[k + 1] - t.leaf_off[k]) * 24 + int(t.class_off[3 * k + 3] - t.class_off[3 * k]) * 12 +
            int(t.gpair_off[g1] - t.gpair_off[g0]) * 9 + (g1 - g0) * 9 + 64)


def rounds(t, budget_bytes):
    budget = int(budget_bytes) or (256 << 20)
    n, k = 0, 0
    while k < t.ntrees:
        used = tree_bytes(t, k)
        k += 1
        while k < t.ntrees and used + tree_bytes(t, k) <= budget:
            used += tree_bytes(t, k)
            k += 1
        n += 1
    return n


def _path(parent, v):
    out = [v]
    while parent[out[-1]] != NONE:
        out.append(parent[out[-1]])
    return out


def _tree(t, k, out):
    n0, n1, l0, l1 = int(t.node_off[k]), int(t.node_off[k + 1]), int(t.leaf_off[k]), int(t.leaf_off[k + 1])
    first, last = t.first[n0:n1].astype(np.int64), t.last[n0:n1].astype(np.int64)
    parent, length = t.parent[n0:n1].tolist(), t.length[n0:n1].tolist()
    internal = np.flatnonzero(t.internal[n0:n1])
    leaf_node = np.flatnonzero(t.internal[n0:n1] == 0).tolist()
    nl, NL = l1 - l0, int(t.leaf_off[-1])
    n = (last - first)[internal]
    for r in range(3):
        c0, c1 = int(t.class_off[3 * k + r]), int(t.class_off[3 * k + r + 1])
        cls = t.leaf_class[r * NL + l0:r * NL + l1].astype(np.int64)
        T = t.class_total[c0:c1].astype(np.int64)[:, None]
        for a in range(0, c1 - c0, 256):                                # (256 classes at a time bound the one-hot matrix)
            b = min(a + 256, c1 - c0)
            pre = np.zeros((b - a, nl + 1), dtype=np.int64)
            pre[:, 1:] = np.cumsum(cls[None, :] == np.arange(a, b)[:, None], axis=1)
            K = pre[:, last[internal]] - pre[:, first[internal]]
            Ts = T[a:b]
            q1 = K.astype(np.float64) / (Ts + (n[None, :] - K)).astype(np.float64)
            q2 = (Ts - K).astype(np.float64) / (Ts + ((nl - n[None, :]) - (Ts - K))).astype(np.float64)
            out["consistency"][c0 + a:c0 + b] = np.maximum(0.0, np.maximum(q1, q2).max(axis=1)) if internal.size else 0.0
    species = t.leaf_species[l0:l1].tolist()
    for g in range(int(t.group_off[k]), int(t.group_off[k + 1])):
        flagged = set()
        for p in range(int(t.gpair_off[g]), int(t.gpair_off[g + 1])):
            a, b = int(t.pair_a[p]), int(t.pair_b[p])
            pa, pb = _path(parent, leaf_node[a]), _path(parent, leaf_node[b])
            on_b = set(pb)
            m = next(v for v in pa if v in on_b)
            if parent[m] == NONE:
                da = 0.0
                for i, v in enumerate(pa):
                    da = length[v] if i == 0 else da + length[v]
                db = 0.0
                for i, v in enumerate(pb):
                    db = length[v] if i == 0 else db + length[v]
                dist = da + db
            else:
                side = pa[:pa.index(m)] + pb[:pb.index(m)]
                dist = length[side[0]]
                for v in side[1:]:
                    dist = dist + length[v]
            out["pair_flag"][p] = 1 if dist > 0 else 0
            if dist > 0:
                flagged.update((a, b))
        if not flagged:
            out["group_node"][g], out["group_mixed"][g] = NONE, 0
            continue
        common = None
        for a in flagged:
            pa = _path(parent, leaf_node[a])
            common = pa if common is None else [v for v in common if v in set(pa)]
        node = common[0]                                                # paths run upwards: the first common node is the deepest
        below = [x for x in range(nl) if node in _path(parent, leaf_node[x])] if nl <= 512 else list(range(int(first[node]), int(last[node])))
        out["group_node"][g] = node
        out["group_mixed"][g] = 1 if len(set(species[x] for x in below if species[x] != NONE)) > 1 else 0


def genetree_run(ctx, t, budget_bytes=0):
    genetree_check(t)
    out = dict(consistency=np.zeros(t.nclasses), pair_flag=np.zeros(t.npairs, dtype=np.uint8), group_node=np.zeros(t.ngroups, dtype=np.uint32),
               group_mixed=np.zeros(t.ngroups, dtype=np.uint8))
    for k in range(t.ntrees):
        _tree(t, k, out)
    out.update(nrounds=rounds(t, budget_bytes), ntrees=t.ntrees, launches=0)
    return out


def runner(tables, budget_bytes=0):
    """What GeneTrees(runner=...) takes."""
    return genetree_run(None, tables, budget_bytes)
