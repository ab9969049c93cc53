"""The attention explanation on the GPU: the segment-select kernels against the tests' own
restatement (``explain_ref``), bitwise; determinism and independence of the chunk length;
the 2015 graph's shape; and ``explain.attention_record(...).explain()`` against the
restatement applied to what the dense record path leaves, and to the reference's dump.

Model-level figures: the exact comparisons carry no tolerance (the per-edge values are the
same launches' bits); against the reference's dump the tie sets are compared at
``DEFAULT_RTOL`` on our side and exactly on the dump's side."""
import numpy as np
import pytest
import torch

from conftest import golden
from gpu_helpers import t

import explain_ref as X

pytestmark = pytest.mark.gpu

POOL = np.array([0.5, 1.0, 1.0 - 2.0 ** -24, 0.25, 3.0, -2.0, 1e-3, 3.0 - 2.0 ** -22], np.float32)
SPECIAL = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
MIXED = [0, 1, 2, 31, 32, 33, 63, 64, 65, 4095, 4096, 4097, 3 * 4096 + 5, 70, 3, 0]
MIXED_NAN = (13, 14)  # all-NaN segments: a long one and a short one
SHORT = [0, 1, 2, 31, 32, 33, 63, 64, 3, 0, 17]
SHORT_NAN = (8,)


def _case(lengths, nan_segs, seed):
    """ptr, per-slot values (about 8 distinct floats, so ties abound, with a sprinkle of
    zeros of both signs, infinities and NaN), ids that are not in slot order."""
    rng = np.random.default_rng(seed)
    ptr = np.zeros(len(lengths) + 1, np.int64)
    np.cumsum(lengths, out=ptr[1:])
    n = int(ptr[-1])
    x = POOL[rng.integers(0, len(POOL), n)]
    sp = rng.random(n) < 0.02
    x[sp] = SPECIAL[rng.integers(0, len(SPECIAL), int(sp.sum()))]
    x[ptr[4]:ptr[4] + 2] = [-0.0, 0.0]
    x[ptr[4] + 2:ptr[5]] = -1.0  # a segment whose maximum is a zero of either sign
    for s in nan_segs:
        x[ptr[s]:ptr[s + 1]] = np.nan
    ids = np.concatenate([rng.permutation(l) + 1000 for l in lengths]).astype(np.int32)
    return ptr, x, ids


def _device_args(ptr, x, ids, variant, cuda, seed=0):
    """(ptr, vals, kwargs) for functional.segment_*: 'plain' reads slot t of a 1-D array,
    'eid' goes through a permutation into the second column of an (n, 2) table
    (ld = 2, off = 1) with the ids given, 'eid1d' through a permutation of a strided view."""
    n = len(x)
    dptr = torch.as_tensor(ptr.astype(np.int32), device=cuda)
    if variant == "plain":
        return dptr, t(x, cuda), {}
    perm = np.random.default_rng(seed + 1).permutation(n)
    tab = np.full((n, 2), 9.0, np.float32)  # column 0 would win every comparison
    tab[perm, 1] = x
    eid = torch.as_tensor(perm.astype(np.int32), device=cuda)
    if variant == "eid":
        return dptr, t(tab, cuda), dict(eid=eid, col=1, ids=torch.as_tensor(ids, device=cuda))
    return dptr, t(tab, cuda)[:, 1], dict(eid=eid)


def _check_ties(got, want):
    mx, n_tie, tp, ti = want
    assert X.same_f32(got.max_val.cpu().numpy(), mx)
    assert np.array_equal(got.count.cpu().numpy(), n_tie)
    assert np.array_equal(got.ptr.cpu().numpy(), tp)
    assert np.array_equal(got.idx[: int(tp[-1])].cpu().numpy(), ti)


@pytest.fixture(scope="module")
def mixed():
    return _case(MIXED, MIXED_NAN, 7)


@pytest.mark.parametrize("variant", ["plain", "eid", "eid1d"])
def test_segment_select_matches_restatement(cuda, msha, mixed, variant):
    from msha_gnn_amd import functional as MF

    ptr, x, ids = mixed
    dptr, vals, kw = _device_args(ptr, x, ids, variant, cuda)
    ref_ids = ids if "ids" in kw else None
    for rtol in (0.0, 2.0 ** -16):
        _check_ties(MF.segment_ties(dptr, vals, rtol=rtol, **kw),
                    X.segment_ties(ptr, x, ref_ids, rtol))
    for k in (1, 5, 64, 65, 128):
        v, i = MF.segment_topk(dptr, vals, k, **kw)
        wv, wi = X.segment_topk(ptr, x, k, ref_ids)
        assert np.array_equal(i.cpu().numpy(), wi), k
        assert X.same_f32(v.cpu().numpy(), wv), k


@pytest.mark.parametrize("lengths,nan_segs", [(SHORT, SHORT_NAN), ([0, 1, 2, 3, 4] * 40, (3,))])
def test_segment_select_short_segments_only(cuda, msha, lengths, nan_segs):
    """Every segment fits its lane group (64 lanes, and 4 lanes at a mean length of 2): the
    long regime has no chunk."""
    from msha_gnn_amd import functional as MF

    ptr, x, ids = _case(lengths, nan_segs, 11)
    dptr, vals, kw = _device_args(ptr, x, ids, "eid", cuda)
    for rtol in (0.0, 2.0 ** -16):
        _check_ties(MF.segment_ties(dptr, vals, rtol=rtol, **kw), X.segment_ties(ptr, x, ids, rtol))
    for k in (1, 5, 65):
        v, i = MF.segment_topk(dptr, vals, k, **kw)
        wv, wi = X.segment_topk(ptr, x, k, ids)
        assert np.array_equal(i.cpu().numpy(), wi) and X.same_f32(v.cpu().numpy(), wv)


def test_segment_select_more_chunks_than_waves(cuda, msha):
    """17,190 chunks of 64 slots: more than the 16,384 waves of the capped chunk grid, so the
    waves stride, and segments of 10,938 and 6,250 chunks, so the first chunk's wave
    combines them over many 64-chunk steps."""
    from msha_gnn_amd import functional as MF

    ptr, x, ids = _case([5, 700_000, 0, 33, 2, 400_000, 70], (3,), 23)
    dptr, vals, kw = _device_args(ptr, x, ids, "eid", cuda)
    want_t = X.segment_ties(ptr, x, ids, 2.0 ** -16)
    want_v, want_i = X.segment_topk(ptr, x, 5, ids)
    for chunk in (64, None):
        _check_ties(MF.segment_ties(dptr, vals, rtol=2.0 ** -16, chunk=chunk, **kw), want_t)
        v, i = MF.segment_topk(dptr, vals, 5, chunk=chunk, **kw)
        assert np.array_equal(i.cpu().numpy(), want_i), chunk
        assert X.same_f32(v.cpu().numpy(), want_v), chunk


def test_segment_select_is_repeatable_and_chunk_independent(cuda, msha, mixed):
    from msha_gnn_amd import functional as MF

    ptr, x, ids = mixed
    dptr, vals, kw = _device_args(ptr, x, ids, "eid", cuda)

    def run(chunk):
        r = MF.segment_ties(dptr, vals, rtol=2.0 ** -16, chunk=chunk, **kw)
        n = int(r.ptr[-1])
        v, i = MF.segment_topk(dptr, vals, 100, chunk=chunk, **kw)
        return [r.max_val.view(torch.int32), r.count, r.ptr, r.idx[:n], v.view(torch.int32), i]

    base = run(None)
    for chunk in (None, 64, 256):
        for a, b in zip(base, run(chunk)):
            assert torch.equal(a, b), chunk


def test_segment_select_captures_into_a_graph(cuda, msha, mixed):
    from msha_gnn_amd import functional as MF

    ptr, x, ids = mixed
    dptr, vals, kw = _device_args(ptr, x, ids, "eid", cuda)
    eager = MF.segment_ties(dptr, vals, rtol=2.0 ** -16, **kw)
    ev, ei = MF.segment_topk(dptr, vals, 5, **kw)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = MF.segment_ties(dptr, vals, rtol=2.0 ** -16, **kw)
        v, i = MF.segment_topk(dptr, vals, 5, **kw)
    g.replay()
    torch.cuda.synchronize()
    n = int(eager.ptr[-1])
    assert torch.equal(r.ptr, eager.ptr) and torch.equal(r.idx[:n], eager.idx[:n])
    assert torch.equal(i, ei) and torch.equal(v.view(torch.int32), ev.view(torch.int32))


# ------------------------------------------------------------------ the 2015 graph ---
@pytest.fixture(scope="module")
def r15(cuda, msha):
    """The 2015 graph (39,179 x 32, 91,283 edges, longest column 5,735 > 4,096) with the
    record of a real eval forward of two heads."""
    from msha_gnn_amd import explain, layers
    from msha_gnn_amd.data import GroupAdjacency

    z, yz = golden("r15_graph.npz"), golden("years.npz")
    n, m = int(z["n"]), int(z["m"])
    g = msha.Graph.from_csr(z["rowptr"].astype(np.int64), z["col"].astype(np.int64), m, cuda)
    torch.manual_seed(3)
    heads = [layers.OursLayer(16, 8, 0.0).to(cuda).eval() for _ in range(2)]
    S, R = torch.rand(n, 16, device=cuda), torch.rand(m, 16, device=cuda)
    city = GroupAdjacency(torch.as_tensor(yz["2015.city"], device=cuda))
    prov = GroupAdjacency(torch.as_tensor(yz["2015.prov"], device=cuda))
    rec = explain.attention_record(heads, g, city, prov, s_input=S, r_input=R)
    return g, rec


def test_r15_rows_and_columns_match_restatement(cuda, msha, r15):
    from msha_gnn_amd import functional as MF
    from msha_gnn_amd.explain import DEFAULT_RTOL

    g, rec = r15
    assert g.n_rows == 39179 and g.n_edges == 91283
    att = rec.att.cpu().numpy()
    rowptr, col = g.rowptr.cpu().numpy(), g.col.cpu().numpy()
    colptr, crow, ceid = (g.colptr.cpu().numpy(), g.csc_row.cpu().numpy(),
                          g.csc_eid.cpu().numpy())
    assert int(np.diff(colptr).max()) > 4096
    ex = rec.explain()
    _check_ties(ex.inter_s, X.segment_ties(rowptr, att, col, DEFAULT_RTOL))
    _check_ties(ex.inter_r, X.segment_ties(colptr, att[ceid], crow, DEFAULT_RTOL))
    # a degree-1 source attends to its recipient alone; every such source is in the tie set
    # of its recipient's column (the reference's value there is exactly 1.0)
    deg1 = np.nonzero(np.diff(rowptr) == 1)[0]
    cols = ex.inter_r.lists()
    for j in range(g.n_cols):
        mine = deg1[col[rowptr[deg1]] == j]
        assert np.isin(mine, cols[j]).all(), j
    exk = rec.explain(k=100)
    for (v, i), want in ((exk.inter_s, X.segment_topk(rowptr, att, 100, col)),
                         (exk.inter_r, X.segment_topk(colptr, att[ceid], 100, crow))):
        assert np.array_equal(i.cpu().numpy(), want[1])
        assert X.same_f32(v.cpu().numpy(), want[0])
    # the other head, through the strided view of the same export
    r0 = MF.segment_ties(g.rowptr, rec.attd[: g.n_edges, 0], ids=g.col, rtol=DEFAULT_RTOL)
    _check_ties(r0, X.segment_ties(rowptr, rec.attd[: g.n_edges, 0].cpu().numpy(), col,
                                   DEFAULT_RTOL))


# ------------------------------------------------------------------ model level ---
def _two_head_case(msha, cuda):
    from test_gpu_ours import _layer_case

    from msha_gnn_amd import layers

    z, layer, inter, city, prov, S, R, _ = _layer_case(msha, cuda, "")
    torch.manual_seed(77)
    other = layers.OursLayer(16, 8, 0.0).to(cuda)
    return z, layer.eval(), other.eval(), inter, city, prov, S.detach(), R.detach()


def _dense_record(heads, S, R, inter, city, prov, n):
    """What the existing dense record path leaves: (Coeff12new, C3, C4) on the host."""
    from msha_gnn_amd import layers

    C3, C4 = torch.zeros(n, n, device=S.device), torch.zeros(n, n, device=S.device)
    with torch.no_grad():
        layers.fused_ours_layer(heads, S, R, layers._graph(inter), city, prov,
                                torch.arange(n, device=S.device), False, True, None, C3, C4)
    return (layers.record_state.Coeff12new.cpu().numpy(), C3.cpu().numpy(), C4.cpu().numpy())


def _same_lists(got, want):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        assert np.array_equal(np.asarray(a), np.asarray(b)), i


def test_explain_matches_dense_record_path_exactly(cuda, msha):
    """Both heads, each as the last of the two (the dense dump keeps the last head):
    tie sets with rtol = 0 and K = 5, all four lists, no tolerance."""
    from msha_gnn_amd import explain

    z, l0, l1, inter, city, prov, S, R = _two_head_case(msha, cuda)
    n, m = z["counts"].shape
    for heads in ([l0, l1], [l1, l0]):
        A, C3, C4 = _dense_record(heads, S, R, inter, city, prov, n)
        rec = explain.attention_record(heads, inter, city, prov, s_input=S, r_input=R)
        got = rec.explain(rtol=0.0, empty_as_all=True).lists()
        _same_lists(got["inter_s"], X.dense_ties(A))
        _same_lists(got["inter_r"], X.dense_ties(np.ascontiguousarray(A.T)))
        _same_lists(got["city"], X.dense_ties(C3))
        _same_lists(got["province"], X.dense_ties(C4))
        assert np.array_equal(rec.c3.cpu().numpy(), C3.max(1))
        assert np.array_equal(rec.c4.cpu().numpy(), C4.max(1))
        gk = rec.explain(k=5).lists()
        for name, D in (("inter_s", A), ("inter_r", np.ascontiguousarray(A.T)), ("city", C3),
                        ("province", C4)):
            wv, wi = X.dense_topk(D, 5)
            # the sparse lists stop at the stored entries: the dense row's zeros are filler
            _same_lists(gk[name], [r[v > 0] for r, v in zip(wi, wv)])
        for batch in (32, 64):
            rb = explain.attention_record(heads, inter, city, prov, batch=batch, s_input=S,
                                          r_input=R)
            assert torch.equal(rb.c3.view(torch.int32), rec.c3.view(torch.int32))
            assert torch.equal(rb.c4.view(torch.int32), rec.c4.view(torch.int32))
            assert torch.equal(rb.att.view(torch.int32), rec.att.view(torch.int32))


def test_explain_matches_reference_dump(cuda, msha):
    """Our explanation at DEFAULT_RTOL against the restatement applied to the reference's
    own dump (ours_record.npz): all 64 rows and 29 columns, city and province lists."""
    from msha_gnn_amd import explain

    z, l0, _, inter, city, prov, S, R = _two_head_case(msha, cuda)
    r = golden("ours_record.npz")
    A = r["rec.coeff12new.1"]
    rec = explain.attention_record(l0, inter, city, prov, s_input=S, r_input=R)
    got = rec.explain(empty_as_all=True).lists()
    assert len(got["inter_s"]) == 64 and len(got["inter_r"]) == 29
    _same_lists(got["inter_s"], X.dense_ties(A))
    _same_lists(got["inter_r"], X.dense_ties(np.ascontiguousarray(A.T)))
    _same_lists(got["city"], X.dense_ties(r["rec.coeff3"]))
    _same_lists(got["province"], X.dense_ties(r["rec.coeff4"]))


def test_find_top_k_dicts_and_names(cuda, msha):
    from msha_gnn_amd import explain

    z, l0, _, inter, city, prov, S, R = _two_head_case(msha, cuda)
    n, m = z["counts"].shape
    rec = explain.attention_record(l0, inter, city, prov, s_input=S, r_input=R)
    plain = explain.find_top_k(rec)
    assert sorted(plain) == ["CityAtt", "InterAttR", "InterAttS", "ProvinceAtt"]
    assert list(plain["InterAttS"]) == list(range(n)) and list(plain["InterAttR"]) == list(range(m))
    assert len(plain["CityAtt"]) == n and len(plain["ProvinceAtt"]) == n
    ls = rec.explain().lists()
    assert plain["InterAttS"][0] == [int(j) for j in ls["inter_s"][0]]
    # the reference's maps: source_index is {"0": name, ...}, recipients index -> name
    s_names = {str(i): f"S{i}" for i in range(n)}
    r_names = [f"R{j}" for j in range(m)]
    named = explain.find_top_k(rec, s_names, r_names)
    for i in (0, n - 1):
        assert named["InterAttS"][i] == [f"R{j}" for j in plain["InterAttS"][i]]
        assert named["CityAtt"][i] == [f"S{j}" for j in plain["CityAtt"][i]]
        assert named["ProvinceAtt"][i] == [f"S{j}" for j in plain["ProvinceAtt"][i]]
    assert named["InterAttR"][3] == [f"S{j}" for j in plain["InterAttR"][3]]
    top = explain.find_top_k(rec, k=3)
    assert all(len(v) <= 3 for v in top["InterAttR"].values())
    assert i in plain["CityAtt"][i]
