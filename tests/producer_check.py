"""The comparison of sdmm_push_training's output with the host-routed
reference (oracle.push_training), shared by the rendered cases of
test_gpu_li.py and the constructed ones of test_gpu_producer_edges.py: all
exact -- leaf, source vertex, stats flag, the bits of the average weight, the
point and normal planes against the vertices' own records, seg against the
reference's per-leaf counts, lost against the reference's."""
import numpy as np


def check_records(out, ref, rec, nv, V, num_nodes, tag, plog=None):
    """out: the dict of STree.push_training (device tensors; seg, lost on the
    host); ref: oracle.push_training's dict in (path, push) order."""
    order = np.argsort(ref["node"], kind="stable")        # the device's leaf order
    for k in ("node", "source", "stats", "w"):
        got = out[k].cpu().numpy()
        want = ref[k][order]
        assert got.shape == want.shape, (tag, k, got.shape, want.shape)
        mism = int(np.sum(got.view(np.uint8) != want.view(np.uint8))) if k == "w" else int(np.sum(got != want))
        if plog is not None:
            plog(f"producer_{tag}_{k}_mismatches", mism, 0, records=int(got.size))
        assert mism == 0, (tag, k)
    src = out["source"].cpu().numpy()
    P = nv.shape[0]
    r = rec.reshape(16, V, P)
    p, d = src // V, src % V
    for i in range(6):
        np.testing.assert_array_equal(out["x"][i].cpu().numpy().view(np.uint32), r[7 + i][d, p].view(np.uint32))
    for i in range(3):
        np.testing.assert_array_equal(out["normal"][i].cpu().numpy().view(np.uint32), r[13 + i][d, p].view(np.uint32))
    counts = np.bincount(ref["node"], minlength=num_nodes)
    np.testing.assert_array_equal(out["seg"], np.concatenate([[0], np.cumsum(counts)]))
    assert out["lost"] == ref["lost"], (tag, out["lost"], ref["lost"])
