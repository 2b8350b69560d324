"""The constructed guiding cases (test_gpu_guiding_pools.py) on the host loop
alone, without a GPU: the loop's bookkeeping (counts, splits on the host tree,
relabelling, readiness, the iteration schedule) runs for real on records of
oracle.push_training; only the mixture is a stand-in that counts its EM
iterations.  Every case's own assertions on HostLoop.log -- that a leaf sat at
the threshold, that the cap held, that each readiness comparison was met from
both sides -- hold here, so a construction that stops reaching its situation
fails on the CPU."""
import copy

import numpy as np
import pytest

import test_gpu_guiding_pools as cases
import vertex_cases as vc
from guiding_host_loop import HostLoop, from_oracle


class _Mix:
    def __init__(self, K):
        self.iterations, self.tag = 0, np.random.default_rng(K).uniform(size=3)

    def init_hemisphere(self, pos, nrm, depth_prior, dist, seed):
        self.tag = np.array([pos.sum(), nrm.sum(), dist + seed])

    def get_state(self):
        return {"scalars": np.array([0.0, 0.0, 0.0, float(self.iterations)])}

    def get_params(self):
        return {k: self.tag for k in ("weights", "mean", "cov", "cholLInv", "detInv", "cdf")}

    def clone(self):
        return copy.deepcopy(self)


class _Samples:
    @classmethod
    def from_numpy(cls, x, w, device=None):
        assert x.shape[0] == 6 and x.shape[1] == w.shape[0]
        return cls()


def _stub(pkg):
    class Stub:
        SDMM, DeviceSamples, STree = _Mix, _Samples, pkg.STree

        @staticmethod
        def em_step_batched_iters(mixes, samples, seg, iterations):
            assert len(mixes) == len(iterations) == len(seg) - 1 and (np.diff(seg) >= 8).all()
            for m, it in zip(mixes, iterations):
                m.iterations += int(it)
    return Stub


class _Model:
    """Stands where the device model stands; answers with the loop's own tables."""

    def __init__(self, pair):
        self.pair = pair

    def node_mixtures(self):
        return self.pair.loop.table()

    @property
    def trained(self):
        return sum(m is not None for m in self.pair.loop.table())

    @property
    def tree(self):
        return self.pair.tree


class _HostPair(cases.Pair):
    def __init__(self, pkg, oracle, gpu, K=16, split_depth=1, split_threshold=200, max_leaf_nodes=2048,
                 saved_per_path=8, init_seed=0x1A17, optimize_async=0):
        self.pkg, self.oracle, self.gpu, self.saved = pkg, oracle, gpu, saved_per_path
        self.tree = pkg.STree(vc.LO, vc.HI)
        self.tree.split_to_depth(split_depth)
        self.loop = HostLoop(pkg, oracle, self.tree, K=K, split_threshold=split_threshold,
                             max_leaf_nodes=max_leaf_nodes, init_seed=init_seed, async_=bool(optimize_async),
                             device="cpu")
        self.g = _Model(self)

    def push(self, rec, nv, seed, path0=0):
        r = from_oracle(self.oracle, self.tree.nodes(), rec, nv, 1, path0, self.saved, seed)
        self.loop.push(r)
        self.loop.update()
        return r

    def compare(self):
        return self.g.trained

    def optimize(self, spp):
        self.loop.optimize(spp)
        return self.loop.log[-1]

    def finish(self):
        self.loop.update()
        return self.compare()


_CASES = [(cases.test_split_threshold, (0,)), (cases.test_split_threshold, (1,)), (cases.test_leaf_cap, ()),
          (cases.test_ready_rules, (0,)), (cases.test_ready_rules, (1,)), (cases.test_iterations_schedule, ()),
          (cases.test_split_of_a_trained_leaf, (0,)), (cases.test_split_of_a_trained_leaf, (1,)),
          (cases.test_jitter_copies_dropped_at_a_split, ()), (cases.test_pool_regrowth_with_live_contents, ()),
          (cases.test_many_nodes, ()), (cases.test_push_that_yields_nothing, ()), (cases.test_wider_mixtures, ())]


@pytest.mark.parametrize("case,args", _CASES, ids=[c.__name__[5:] + "".join(f"-{a}" for a in args) for c, args in _CASES])
def test_case_reaches_its_situation(pkg, oracle, monkeypatch, case, args):
    monkeypatch.setattr(cases, "Pair", _HostPair)
    case(_stub(pkg), oracle, "cpu", *args)


def test_quiet_positions_give_one_record_each(oracle):
    """quiet: one own-leaf record per path and no copy; loud: copies reach
    neighbours, and their stored point lies outside the leaf that got them."""
    rng = np.random.default_rng(0)
    nodes = vc.unit_tree(oracle, 1)
    for o in range(8):
        rec, nv = cases.paths(rng, cases.quiet(rng, o, 400))
        r = from_oracle(oracle, nodes, rec, nv, 1, 0, 8, 77 + o)
        assert r["node"].shape[0] == 400 and r["stats"].all() and np.unique(r["node"]).size == 1
        rec, nv = cases.paths(rng, cases.loud(rng, o, 400))
        r = from_oracle(oracle, nodes, rec, nv, 1, 0, 8, 77 + o)
        copies = ~r["stats"]
        assert copies.sum() > 200
        found = oracle.stree_find(nodes[0], nodes[1], np.ascontiguousarray(r["x"][:3].T))
        assert (found[copies] != r["node"][copies]).all() and (found[~copies] == r["node"][~copies]).all()
