"""The reference schedule of the guiding model: the plugin's optimize() loop
(volpath_sdmm.cpp:244-312, :411-507) on the host side of the C ABI, the
yardstick sdmm_guiding_* (guiding.hip) is held to bitwise.

Per leaf it keeps the records (context->data) and the stats positions
(context->stats) in arrival order.  optimize(spp):

  split      while leaf_nodes <= max_leaf_nodes (checked once, :253): every
             leaf by its OWN stats positions, split_leaf_recurse_many on the
             host tree (a whole-tree split of all leaves' positions would hand
             a position on a leaf boundary to both leaves; whole_tree_check
             asserts that the two forms agree where that never happens)
  hand down  a split leaf's mixture (and conditioner) is copied to every new
             leaf below it, its records and stats positions move to the leaf
             oracle.stree_find gives them in the new tree; one found outside
             the split leaf's subtree is dropped (jmm createChildNode keeps
             what the child's box holds)
  ready      canBeOptimized (:140-149): (total_spp > 12 or n_data > 1000),
             leaf, n_stats >= 64, n_data >= 8
  train      a new leaf starts from its first K/8 records (hemisphere init,
             spatial distance 3 hmax(diag) / (K/8), 0.1 hmax(diag) when async);
             2 EM iterations while iterations_run < 4, else 1 (async: 1); the
             leaf's records are dropped, its stats stay
  async      the renders read the conditioners, refreshed by update() from
             the leaves the previous optimize stepped (:180-242)

Records enter through push(): host arrays in leaf order, a leaf's records in
(path, push) order -- from_device() of an STree.push_training result, or
from_oracle() of oracle.push_training on constructed vertices.  Every
optimize() appends its own tables to .log, from which a test asserts that
the situation it was built for occurred.
"""
import numpy as np


def from_device(out):
    """STree.push_training's dict -> host records."""
    return {"x": np.stack([t.cpu().numpy() for t in out["x"]]),
            "normal": np.stack([t.cpu().numpy() for t in out["normal"]]),
            "w": out["w"].cpu().numpy(), "stats": out["stats"].cpu().numpy().astype(bool),
            "node": out["node"].cpu().numpy()}


def from_oracle(oracle, nodes, rec, nv, V, path0, saved, seed):
    """oracle.push_training on vertices (rec, nv), stably sorted by leaf, with
    the point and normal planes taken from the vertices' own records."""
    aabb, child = nodes[0], nodes[1]
    ref = oracle.push_training(aabb, child, rec, nv, V, path0, saved, seed)
    order = np.argsort(ref["node"], kind="stable")
    src = ref["source"][order]
    r = rec.reshape(16, V, nv.shape[0])
    p, d = src // V, src % V
    return {"x": np.stack([r[7 + i][d, p] for i in range(6)]).reshape(6, -1),
            "normal": np.stack([r[13 + i][d, p] for i in range(3)]).reshape(3, -1),
            "w": ref["w"][order], "stats": ref["stats"][order].astype(bool), "node": ref["node"][order],
            "lost": ref["lost"]}


def _subtree(child, v):
    out, stack = [], [v]
    while stack:
        i = stack.pop()
        out.append(i)
        if child[i, 0] >= 0:
            stack += [int(child[i, 0]), int(child[i, 1])]
    return np.asarray(out)


class HostLoop:
    def __init__(self, pkg, oracle, tree, K=16, split_threshold=4000, max_leaf_nodes=2048, init_seed=0x1A17,
                 depth_prior=0.01, async_=False, whole_tree_check=False, device="cuda"):
        self.pkg, self.oracle, self.tree = pkg, oracle, tree
        self.K, self.split_threshold, self.max_leaf_nodes = K, split_threshold, max_leaf_nodes
        self.init_seed, self.depth_prior, self.async_ = init_seed, depth_prior, async_
        self.whole_tree_check, self.device = whole_tree_check, device
        self.data = {}      # leaf -> list of (x (6, n), normal (3, n), w (n,))
        self.stats = {}     # leaf -> list of positions (3, n)
        self.mix = {}
        self.cond = {}      # async: leaf -> conditioner
        self.pending = []   # async: the leaves the running EM steps
        self.total_spp = 0
        self.log = []

    # ---- tables
    def n_data(self, v):
        return sum(int(c[2].shape[0]) for c in self.data.get(v, []))

    def n_stats(self, v):
        return sum(int(p.shape[1]) for p in self.stats.get(v, []))

    def table(self):
        """Per node: the mixture the renders use (the conditioner when async)."""
        tab = self.cond if self.async_ else self.mix
        return [tab.get(i) for i in range(self.tree.num_nodes)]

    def mixtures(self):
        return [self.mix.get(i) for i in range(self.tree.num_nodes)]

    # ---- a pass's records
    def push(self, rec):
        node = rec["node"]
        assert (np.diff(node) >= 0).all(), "records must come in leaf order"
        leaves, start = np.unique(node, return_index=True)
        end = list(start[1:]) + [node.shape[0]]
        for v, a, b in zip(leaves.tolist(), start.tolist(), end):
            self.data.setdefault(v, []).append((rec["x"][:, a:b], rec["normal"][:, a:b], rec["w"][a:b]))
            st = rec["stats"][a:b]
            if st.any():
                self.stats.setdefault(v, []).append(rec["x"][:3, a:b][:, st])

    def update(self):
        for v in self.pending:
            self.cond[v] = self.mix[v].clone()
        self.pending = []

    # ---- optimize()
    def _split(self, entry):
        tree = self.tree
        aabb, child, axis = tree.nodes()
        if tree.leaf_nodes > self.max_leaf_nodes:
            entry["capped"] = True
            return
        leaves = [v for v in sorted(self.stats) if child[v, 0] < 0 and self.n_stats(v) > self.split_threshold]
        entry["over_threshold"] = list(leaves)
        if not leaves:
            return
        pos = [np.concatenate(self.stats[v], 1) for v in leaves]
        if self.whole_tree_check:
            # the whole-tree form on a copy: every leaf's positions at once
            other = self.pkg.STree(aabb[0, :3], aabb[0, 3:])
            other.set_nodes(aabb, child, axis)
            allpos = np.concatenate([np.concatenate(self.stats[v], 1) for v in sorted(self.stats)], 1)
            other.split_leaves(allpos, threshold=self.split_threshold, max_leaf_nodes=self.max_leaf_nodes)
        tree.split_leaf_recurse_many(leaves, pos, self.split_threshold)
        if self.whole_tree_check:
            for a, b in zip(tree.nodes(), other.nodes()):
                np.testing.assert_array_equal(a, b, err_msg="per-leaf and whole-tree splits differ")

    def _hand_down(self, old_n, entry):
        aabb, child, _ = self.tree.nodes()
        find = lambda pts: self.oracle.stree_find(aabb, child, np.ascontiguousarray(pts.T))
        for v in sorted(set(self.data) | set(self.stats) | set(self.mix) | set(self.cond)):
            if v >= old_n or child[v, 0] < 0:
                continue
            entry["split"].append(v)
            sub = _subtree(child, v)
            leaves = [int(i) for i in sub if child[i, 0] < 0]
            for tab in (self.mix, self.cond):
                parent = tab.pop(v, None)
                if parent is not None:
                    for c in leaves:
                        tab[c] = parent.clone()
                    entry["inherited"] += [(v, c) for c in leaves] if tab is self.mix else []
            recs = self.data.pop(v, [])
            if recs:
                x = np.concatenate([r[0] for r in recs], 1)
                nr = np.concatenate([r[1] for r in recs], 1)
                w = np.concatenate([r[2] for r in recs])
                node = find(x[:3])
                node[~np.isin(node, sub)] = -1     # outside the split leaf: dropped
                entry["dropped"] += int((node < 0).sum())
                for c in np.unique(node[node >= 0]).tolist():
                    sel = node == c
                    self.data.setdefault(c, []).append((x[:, sel], nr[:, sel], w[sel]))
            pos = self.stats.pop(v, [])
            if pos:
                ps = np.concatenate(pos, 1)
                pnode = find(ps)
                pnode[~np.isin(pnode, sub)] = -1
                entry["dropped_stats"] += int((pnode < 0).sum())
                for c in np.unique(pnode[pnode >= 0]).tolist():
                    self.stats.setdefault(c, []).append(ps[:, pnode == c])

    def optimize(self, spp):
        import torch
        pkg, tree, K = self.pkg, self.tree, self.K
        self.update()       # async: no split while an EM runs
        entry = {"total_spp": self.total_spp, "split": [], "inherited": [], "dropped": 0, "dropped_stats": 0,
                 "capped": False, "over_threshold": [], "ready": [], "fresh": [], "iterations": [],
                 "n_stats_before": {v: self.n_stats(v) for v in self.stats}}
        self.log.append(entry)
        old_n = tree.num_nodes
        self._split(entry)
        if tree.num_nodes != old_n:
            self._hand_down(old_n, entry)
        aabb, child, _ = tree.nodes()
        entry["n_data"] = {v: self.n_data(v) for v in self.data}
        entry["n_stats"] = {v: self.n_stats(v) for v in self.stats}
        ready = []
        for v in sorted(self.data):
            n_data, n_stats = self.n_data(v), self.n_stats(v)
            if (self.total_spp > 12 or n_data > 1000) and child[v, 0] < 0 and n_stats >= 64 and n_data >= 8:
                ready.append(v)
        entry["ready"] = list(ready)
        out = {"leaves": tree.leaf_nodes, "optimized": len(ready), "records": sum(entry["n_data"].values())}
        entry["stats"] = out
        self.total_spp += spp             # m_totalSpp grows after optimize() (volpath_sdmm.cpp:495-506)
        if not ready:
            return out
        segs, xs, ws, its, mixes = [0], [], [], [], []
        for v in ready:
            recs = self.data.pop(v)
            x = np.concatenate([r[0] for r in recs], 1)
            nr = np.concatenate([r[1] for r in recs], 1)
            w = np.concatenate([r[2] for r in recs])
            if v not in self.mix:
                m = pkg.SDMM(K)
                diag = np.max(aabb[v, 3:] - aabb[v, :3]).astype(np.float32)
                if self.async_:
                    diag = np.float32(0.1) * diag
                npos = K // 8
                m.init_hemisphere(np.ascontiguousarray(x[:3, :npos].T), np.ascontiguousarray(nr[:, :npos].T),
                                  self.depth_prior, 3.0 * float(diag) / npos, self.init_seed + v)
                self.mix[v] = m
                entry["fresh"].append(v)
            m = self.mix[v]
            its.append(1 if self.async_ else (2 if m.get_state()["scalars"][3] < 4 else 1))
            mixes.append(m)
            xs.append(x)
            ws.append(w)
            segs.append(segs[-1] + int(w.shape[0]))
        entry["iterations"] = list(its)
        samples = pkg.DeviceSamples.from_numpy(np.concatenate(xs, 1), np.concatenate(ws), device=self.device)
        pkg.em_step_batched_iters(mixes, samples, np.asarray(segs, np.int64), np.asarray(its, np.int32))
        if torch.cuda.is_available():
            torch.cuda.synchronize()
        self.pending = list(ready)
        return out


def assert_same_mixtures(ref, got):
    """Per node: the same nodes hold a mixture, and every mixture's parameters
    and EM state are equal bitwise.  Returns the number of mixtures."""
    assert len(got) == len(ref)
    n = 0
    for i, (r, m) in enumerate(zip(ref, got)):
        assert (r is None) == (m is None), i
        if r is None:
            continue
        n += 1
        pr, pm = r.get_params(), m.get_params()
        for k in ("weights", "mean", "cov", "cholLInv", "detInv", "cdf"):
            np.testing.assert_array_equal(pr[k], pm[k], err_msg=f"node {i} {k}")
        sr, sm = r.get_state(), m.get_state()
        for k in sr:
            np.testing.assert_array_equal(sr[k], sm[k], err_msg=f"node {i} state {k}")
    return n
