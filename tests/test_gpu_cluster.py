"""Token clustering on the GPU (csrc/cluster.hip; ops.cluster_pages, PageCorpus.from_clustered / append_clustered):
the fused kernel against ops.cluster_reference run on the CPU (equal lists, offsets and labels), repeatability, graph capture, the
clustered corpus against from_pooled fed with the kernel's lists (equal bits in planes, words and scores), and the clustered corpus
as the first stage of a two-stage search against the window-pooled one.  Sections 4 to 8 put the kernel where a wrong sum, a wrong
compare or a wrong index would show: near-tie pages (tests/test_cluster_host.py counts the labels that another arithmetic moves on
them), the rule's edges, the geometry's boundaries, misaligned and strided sources, mask forms, two streams and a regrown workspace.
Every comparison there is torch.equal against the CPU reference: there is no tolerance in this file."""
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import cluster_cases as cc  # noqa: E402

pytestmark = pytest.mark.gpu

KINDS = ("bf16", "fp32", "fp8")
DTYPES = (torch.float32, torch.bfloat16, torch.float16)
# (lp_src, ls, d, n): the shapes of the rule's table; 700 / 312 and 700 / 313 sit on the two sides of the centroid threshold (LDS
# against the workspace); 33 / 9 with 515 pages is more pages than the launch's grid holds workgroups (512)
SHAPES = ((7, 3, 128, 4), (33, 9, 64, 4), (300, 40, 20, 4), (225, 57, 128, 4), (1030, 258, 128, 6))
EXTRA = ((700, 312, 32, 3, torch.float32), (700, 313, 32, 3, torch.bfloat16), (33, 9, 64, 515, torch.float16))
ITERS = (0, 1, 6)


@pytest.fixture(scope="module")
def dev():
    import evdr_amd  # noqa: F401
    return torch.device("cuda:0")


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.contiguous().view(torch.int32)


def check_against_reference(dev, lp, ls, d, n, dtype):
    from evdr_amd import ops
    P, pm = cc.case(lp, ls, d, dtype, n)
    _, history = cc.reference(lp, ls, d, dtype, n, ITERS[-1])
    moved = cc.changes(history)
    print(f"lp_src={lp} ls={ls} d={d} n={n} {dtype}: labels changed per iteration {moved}")
    if lp != 7:                                                        # the case must exercise the loop: kept for its geometry only
        assert any(a > 0 and b > 0 for a, b in zip(moved[:-1], moved[1:])), moved
    Pd, pmd = P.to(dev), pm.to(dev)
    for iters in ITERS:
        (wmem, woff, wlab), _ = cc.reference(lp, ls, d, dtype, n, iters)
        mem, off, lab = ops.cluster_pages(Pd, pmd, ls=ls, iters=iters, return_labels=True)
        assert mem.dtype == off.dtype == lab.dtype == torch.int32 and mem.device == off.device == lab.device == dev
        assert tuple(mem.shape) == (n, lp) and tuple(off.shape) == (n, ls + 1) and tuple(lab.shape) == (n, lp)
        mem, off, lab = mem.cpu(), off.cpu(), lab.cpu()
        print(f"  iters={iters}: {int((lab != wlab).sum())} labels, {int((off != woff).sum())} offsets, {int((mem != wmem).sum())} members differ")
        assert torch.equal(lab, wlab), (iters, "labels")
        assert torch.equal(off, woff), (iters, "offsets")
        assert torch.equal(mem, wmem), (iters, "members")
        mem2, off2 = ops.cluster_pages(Pd, pmd, ls=ls, iters=iters)  # without the labels
        assert torch.equal(mem2.cpu(), wmem) and torch.equal(off2.cpu(), woff)


# ---- 1. the kernel against the rule ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES, ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("lp,ls,d,n", SHAPES)
def test_cluster_pages_equals_reference(dev, lp, ls, d, n, dtype):
    check_against_reference(dev, lp, ls, d, n, dtype)


@pytest.mark.parametrize("lp,ls,d,n,dtype", EXTRA, ids=("lds312", "workspace313", "grid515"))
def test_cluster_pages_equals_reference_at_the_thresholds(dev, lp, ls, d, n, dtype):
    check_against_reference(dev, lp, ls, d, n, dtype)


def test_cluster_pages_without_a_mask_and_by_factor(dev):
    from evdr_amd import ops
    P, _ = cc.case(225, 57, 128, torch.float32, 4)
    want = ops.cluster_reference(P, None, 57, 3)
    got = ops.cluster_pages(P.to(dev), None, factor=4, iters=3, return_labels=True)     # ceil(225 / 4) = 57
    assert all(torch.equal(g.cpu(), w) for g, w in zip(got, want))
    mem, off = ops.cluster_pages(P[:0].to(dev), None, ls=57)
    assert tuple(mem.shape) == (0, 225) and tuple(off.shape) == (0, 58)


def test_two_launches_give_the_same_bits(dev):
    from evdr_amd import ops
    P, pm = (t.to(dev) for t in cc.case(225, 57, 128, torch.bfloat16, 4))
    a = ops.cluster_pages(P, pm, ls=57, iters=6, return_labels=True)
    b = ops.cluster_pages(P, pm, ls=57, iters=6, return_labels=True)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_graph_capture_and_replay(dev):
    """One launch, no allocation and no synchronisation inside the C ABI: a captured graph replays the clustering and tracks its input."""
    from evdr_amd import ops
    P, pm = cc.case(225, 57, 128, torch.float32, 4)
    Ps, pmd = P.to(dev).clone(), pm.to(dev)
    side = torch.cuda.Stream(device=dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):                                      # warm-up outside capture: kernel attributes, the workspace
        ops.cluster_pages(Ps, pmd, ls=57, iters=6, return_labels=True)
    torch.cuda.current_stream(dev).wait_stream(side)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        out = ops.cluster_pages(Ps, pmd, ls=57, iters=6, return_labels=True)
    P2 = P.flip(0)
    pm2 = pm.flip(0)
    Ps.copy_(P2.to(dev))
    pmd.copy_(pm2.to(dev))
    g.replay()
    torch.cuda.synchronize()
    want = ops.cluster_reference(P2, pm2, 57, 6)
    assert all(torch.equal(x.cpu(), w) for x, w in zip(out, want))
    direct = ops.cluster_pages(Ps, pmd, ls=57, iters=6, return_labels=True)
    assert all(torch.equal(x, y) for x, y in zip(out, direct))


# ---- 2. the fused path ------------------------------------------------------------------------------------------------------------------
def corpus_dtype(kind: str):
    from evdr_amd import ops
    return {"bf16": torch.bfloat16, "fp32": torch.float32, "fp8": ops.FP8}[kind]


def assert_same_corpus(a, b):
    assert a.n_pages == b.n_pages and a.lp == b.lp and a.nplanes == b.nplanes and a.fp8 == b.fp8 and a.planes.dtype == b.planes.dtype
    assert a.idx_base == b.idx_base
    view = torch.uint8 if a.fp8 else torch.int16
    assert torch.equal(a.planes.view(view), b.planes.view(view))
    assert torch.equal(a.tilemask, b.tilemask)
    assert torch.equal(a.pageflags, b.pageflags)
    assert (a.shift is None) == (b.shift is None) and (a.shift is None or torch.equal(a.shift, b.shift))
    assert (a.amax is None) == (b.amax is None) and (a.amax is None or torch.equal(a.amax, b.amax))


def assert_same_scores(kind: str, a, b, dev, d: int):
    gen = torch.Generator(device=dev).manual_seed(77)
    Q = torch.nn.functional.normalize(torch.randn((3, 8, d), generator=gen, device=dev), dim=-1)
    Q = Q.bfloat16() if kind == "bf16" else Q
    qm = torch.arange(8, device=dev)[None, :] < torch.tensor([[8], [3], [5]], device=dev)
    assert torch.equal(bits(a.score(Q, qm)), bits(b.score(Q, qm)))
    (sa, ia), (sb, ib) = a.topk(Q, qm, 3), b.topk(Q, qm, 3)
    assert torch.equal(bits(sa), bits(sb)) and torch.equal(ia, ib)


@pytest.mark.parametrize("kind", KINDS)
def test_from_clustered_equals_from_pooled_of_the_clustered_lists(dev, kind):
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus
    lp, ls, d, n = 33, 9, 64, 4
    P, pm = (t.to(dev) for t in cc.case(lp, ls, d, torch.bfloat16 if kind == "bf16" else torch.float32, n))
    dt = corpus_dtype(kind)
    for kw in (dict(ls=ls, iters=6), dict(factor=4, iters=2)):        # ceil(33 / 4) = 9
        a = PageCorpus.from_clustered(P, pm, dtype=dt, idx_base=40, chunk_pages=3, **kw)             # two chunks: 3 pages + 1
        b = PageCorpus.from_pooled(P, pm, *ops.cluster_pages(P, pm, **kw), dtype=dt, idx_base=40)
        assert a.lp == ls and a.capacity == a.n_pages == n
        assert_same_corpus(a, b)
        assert_same_scores(kind, a, b, dev, d)
    a = PageCorpus.from_clustered(P, pm, ls=ls)                       # the default kind and chunk
    assert a.planes.dtype == (torch.bfloat16 if kind == "bf16" else torch.float16) and a.n_pages == n


@pytest.mark.parametrize("kind", KINDS)
def test_append_clustered_behind_earlier_views(dev, kind):
    from evdr_amd.corpus import PageCorpus
    lp, ls, d, n = 225, 57, 128, 4
    P, pm = (t.to(dev) for t in cc.case(lp, ls, d, torch.bfloat16 if kind == "bf16" else torch.float32, n))
    dt = corpus_dtype(kind)
    c = PageCorpus.from_clustered(P[:1], pm[:1], ls=ls, iters=3, dtype=dt, capacity=n + 1, idx_base=10)
    view = c.shard(0, 1)                                              # made before the corpus grows
    assert c.append_clustered(P[1:], pm[1:], iters=3, chunk_pages=2) == 11
    assert c.n_pages == n and c.capacity == n + 1 and view.n_pages == 1
    full = PageCorpus.from_clustered(P, pm, ls=ls, iters=3, dtype=dt, idx_base=10)
    assert_same_corpus(c, full)
    assert_same_corpus(view, full.shard(0, 1))
    assert_same_scores(kind, c, full, dev, d)


# ---- 3. the clustered corpus as a first stage -------------------------------------------------------------------------------------------
def test_clustered_first_stage_beats_windows(dev):
    """64 structured pages (12 prototypes in shuffled order, 90 valid patches, page 3 with 40) pooled to 12 tokens; 64 queries of eight
    noisy patches of their page; k = 10 out of 16 candidates.  Windows average unrelated neighbours, clusters average copies of one
    prototype: the CPU statement of both (ops.pool_reference of ops.cluster_reference's lists, fp32 scores of the bf16-rounded
    tensors) gives recall 0.86 against 0.67 on this seed; the margin asked for is half that gap, because the coarse corpora hold the
    reference's bits and only the bf16 scoring differs.  The planted page is first either way."""
    from evdr_amd import ops
    from evdr_amd.corpus import PageCorpus, TwoStageRetriever
    P, pm, Q = (t.to(dev) for t in cc.two_stage_case())
    P, Q = P.bfloat16(), Q.bfloat16()
    n = P.shape[0]
    exact = PageCorpus.from_tensor(P, pm)
    want = exact.topk(Q, None, 10)[1]
    recall = {}
    for name, coarse in (("windows", PageCorpus.from_pooled(P, pm, *ops.pool_groups_windows(96, 8))),
                         ("clustered", PageCorpus.from_clustered(P, pm, ls=12, iters=8))):
        assert coarse.lp == 12 and coarse.n_pages == n
        _, idx = TwoStageRetriever(coarse, exact).search(Q, None, k=10, candidates=16)
        assert idx[:, 0].tolist() == list(range(n)), name             # planted top-1 = 1.0
        recall[name] = sum(len(set(a) & set(b)) for a, b in zip(idx.tolist(), want.tolist())) / (10 * n)
    print(f"recall@10 of a 16-candidate first stage: {recall}")
    assert recall["clustered"] >= recall["windows"] + 0.1, recall


# ---- 4. near ties: where the arithmetic decides the label -------------------------------------------------------------------------------
def assert_equals_reference(got, want, what):
    got = [g.cpu() for g in got]
    print(f"{what}: {[int((g != w).sum()) for g, w in zip(got, want)]} members / offsets / labels differ")
    for name, g, w in zip(("members", "offsets", "labels"), got, want):
        assert g.dtype == torch.int32 and torch.equal(g, w), (what, name)
    return got


def check_built(dev, builder, args, iters_list):
    """ops.cluster_pages on the GPU against the shared CPU reference of cc.built(builder, *args); the kernel's (members, offsets,
    labels) of the last iteration count, on the CPU."""
    from evdr_amd import ops
    P, pm, ls = cc.built(builder, *args)
    Pd, pmd = P.to(dev), None if pm is None else pm.to(dev)
    for iters in iters_list:
        want, _ = cc.built_reference(builder, args, iters)
        got = assert_equals_reference(ops.cluster_pages(Pd, pmd, ls=ls, iters=iters, return_labels=True), want,
                                      f"{builder.__name__}{args} iters={iters}")
    return got


@pytest.mark.parametrize("args", cc.NEAR_TIE, ids=lambda a: f"{a[0]}-{a[1]}-{a[2]}-{str(a[3])[6:]}")
def test_near_tie_pages_equal_reference(dev, args):
    """Patches within a few ulps of one row: test_cluster_host.py::test_near_tie_cases_tell_other_arithmetics_apart shows that an fp64
    dot, a left-to-right sum, fused multiply-adds or fp64 centroids each move labels on these very pages."""
    check_built(dev, cc.near_tie_case, args, (1, cc.NEAR_TIE_ITERS))


def test_from_clustered_of_near_ties_equals_from_pooled_of_the_reference_lists(dev):
    """The lists come from ops.cluster_reference on the CPU, not from the kernel: a wrong list inside from_clustered shows."""
    from evdr_amd.corpus import PageCorpus
    args = cc.NEAR_TIE[0]
    P, pm, ls = cc.built(cc.near_tie_case, *args)
    (mem, off, _), _ = cc.built_reference(cc.near_tie_case, args, cc.NEAR_TIE_ITERS)
    Pd = P.to(dev)
    a = PageCorpus.from_clustered(Pd, None, ls=ls, iters=cc.NEAR_TIE_ITERS, dtype=torch.bfloat16, idx_base=40, chunk_pages=3)
    b = PageCorpus.from_pooled(Pd, None, mem.to(dev), off.to(dev), dtype=torch.bfloat16, idx_base=40)
    assert_same_corpus(a, b)
    assert_same_scores("bf16", a, b, dev, args[2])


# ---- 5. the rule's edges through the kernel ---------------------------------------------------------------------------------------------
def test_ties_emptied_groups_and_signed_zeros_through_the_kernel(dev):
    """The inputs and the literal lists of test_cluster_host.py::test_ties_go_to_the_lower_group_and_an_emptied_group_keeps_its_centroid."""
    for iters in (1, 2, 5):
        mem, off, lab = check_built(dev, cc.tie_page, (), (iters,))
        assert lab.tolist() == [[0, 0, 0, 0]] and off.tolist() == [[0, 4, 4]] and mem.tolist() == [[0, 1, 2, 3]]
    _, _, lab = check_built(dev, cc.signed_zero_page, (), (1,))
    assert lab.tolist() == [[0, 0, 1, 1]]


def test_nan_patches_get_label_zero_through_the_kernel(dev):
    """The inputs and the statements of test_cluster_host.py::test_a_nan_patch_gets_label_zero."""
    _, _, lab = check_built(dev, cc.nan_patch_page, (), (0, 1))
    assert int(lab[0, 4]) == 0 and all(int(lab[0, p]) in (0, 1) for p in (0, 1, 2, 3, 5))
    _, off, lab = check_built(dev, cc.all_nan_page, (), (1, 2))
    assert lab.tolist() == [[0] * 5] and off.tolist() == [[0, 5, 5]]


@pytest.mark.parametrize("dtype", (torch.float32, torch.float16), ids=("float32", "float16"))
def test_infinite_patches(dev, dtype):
    check_built(dev, cc.inf_page, (dtype,), (1, 3))


@pytest.mark.parametrize("lp,ls,d", ((300, 40, 64), (700, 313, 32)))
def test_identical_patches_all_tie_into_group_zero(dev, lp, ls, d):
    """Every patch ties; groups 1.. are emptied by the first assign and keep their centroids over the next two."""
    for iters in (1, 3):
        mem, off, lab = check_built(dev, cc.identical_page, (lp, ls, d), (iters,))
        assert not lab.any() and mem[0].tolist() == list(range(lp)) and off[0].tolist() == [0] + [lp] * ls


@pytest.mark.parametrize("lp,ls,d", ((33, 9, 64), (300, 40, 64)))
def test_two_rows_repeated_alternately(dev, lp, ls, d):
    check_built(dev, cc.alternating_page, (lp, ls, d), (1, 3))


@pytest.mark.parametrize("dtype,scale", ((torch.float32, 1e-25), (torch.float32, 1e25), (torch.float16, 3e4)), ids=("tiny", "overflow", "fp16-3e4"))
def test_magnitudes_follow_the_reference(dev, dtype, scale):
    """Squares that are denormal or zero (the + 1e-12 is the denominator), a sum of squares that overflows, fp16 under its maximum: the
    reference decides what is right."""
    check_built(dev, cc.scaled_case, (225, 57, 128, dtype, scale), (1, 3))


# ---- 6. geometry -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scattered", (False, True), ids=("prefix", "scattered"))
def test_valid_counts_on_wave_and_workgroup_boundaries(dev, scattered):
    check_built(dev, cc.boundary_case, (scattered,), (0, 1, 3))


@pytest.mark.parametrize("lp,ls,d", [(lp, ls, 24) for lp in (1, 2, 3, 5) for ls in (1, 3)] + [(33, 1, 64), (40, 4096, 16)])
def test_short_pages_one_group_and_more_groups_than_patches(dev, lp, ls, d):
    check_built(dev, cc.plain_case, (lp, ls, d, 2, False), (0, 2))
    check_built(dev, cc.plain_case, (lp, ls, d, 4, True), (0, 2))


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda v: str(v).replace("torch.", ""))
@pytest.mark.parametrize("d", (1, 7, 8, 100, 127, 128))
def test_embedding_widths(dev, d, dtype):
    check_built(dev, cc.plain_case, (33, 9, d, 4, True, dtype), (0, 3))


def test_the_most_iterations_the_header_allows(dev):
    check_built(dev, cc.plain_case, (33, 9, 64, 4, True), (64,))


def test_the_largest_page_the_header_allows(dev):
    """lp_src = 65535 with ls = 4096 and no iteration (the start labels at the largest i * g), then one iteration at ls = 16: the sizes
    test_cluster_host.py::test_the_largest_page_the_header_allows_is_quick_on_the_cpu times."""
    from evdr_amd import ops
    try:
        check_built(dev, cc.plain_case, (65535, 4096, 8, 1, False), (0,))
        check_built(dev, cc.plain_case, (65535, 16, 8, 1, False), (1,))
    finally:
        torch.cuda.synchronize()
        ops._cluster_ws.clear()                                       # 512 slices of 65535 labels + 4096 centroids: 1.2 GB, not kept


def test_three_rounds_of_the_grid_walk(dev):
    check_built(dev, cc.grid_walk_case, (), (1, 3))


# ---- 7. source access and masks -----------------------------------------------------------------------------------------------------------
def small_case(dtype):
    """(P, pmask, the reference after ITERS[-1] iterations) of the (33, 9, 64) case of section 1."""
    P, pm = cc.case(33, 9, 64, dtype, 4)
    return P, pm, cc.reference(33, 9, 64, dtype, 4, ITERS[-1])[0]


@pytest.mark.parametrize("dtype", DTYPES, ids=lambda v: str(v).replace("torch.", ""))
def test_misaligned_base_pointer(dev, dtype):
    """d % 8 == 0, but the storage starts one element into its buffer: the element-wise instances."""
    from evdr_amd import ops
    P, pm, want = small_case(dtype)
    buf = torch.empty(P.numel() + 1, dtype=dtype, device=dev)
    Pd = buf[1:].view(P.shape)
    Pd.copy_(P)
    assert Pd.is_contiguous() and Pd.data_ptr() % 16 != 0
    assert_equals_reference(ops.cluster_pages(Pd, pm.to(dev), ls=9, iters=ITERS[-1], return_labels=True), want, f"misaligned {dtype}")


@pytest.mark.parametrize("gap", (8, 3), ids=("aligned", "unaligned"))
@pytest.mark.parametrize("dtype", (torch.float32, torch.bfloat16), ids=("float32", "bfloat16"))
def test_c_abi_direct_with_a_page_stride(dev, dtype, gap):
    """evdr_cluster_pages through ctypes on pages that are rows of a wider buffer, NaN between them: src_stride = lp * d + 8 keeps every
    page 16-byte aligned, + 3 does not."""
    from evdr_amd import _lib as L, ops
    P, pm, want = small_case(dtype)
    n, lp, d = P.shape
    stride = lp * d + gap
    buf = torch.full((n, stride), float("nan"), dtype=dtype, device=dev)
    buf[:, :lp * d] = P.view(n, -1).to(dev)
    assert (stride * buf.element_size()) % 16 == (0 if gap == 8 else 12 if dtype is torch.float32 else 6)
    lib = L.load()
    ws = torch.empty(lib.evdr_cluster_pages_workspace(lp, 9), dtype=torch.uint8, device=dev)
    mem, lab = (torch.empty((n, lp), dtype=torch.int32, device=dev) for _ in range(2))
    off = torch.empty((n, 10), dtype=torch.int32, device=dev)
    pmd = pm.to(dev)
    L.check(lib.evdr_cluster_pages(L.ptr(buf), ops._SRC_DTYPE[dtype], L.ptr(pmd), n, lp, d, stride, 9, ITERS[-1], L.ptr(mem), L.ptr(off),
                                   L.ptr(lab), L.ptr(ws), ws.numel(), L.current_stream_handle(dev)))
    assert_equals_reference((mem, off, lab), want, f"stride {stride} {dtype}")
    assert bool(torch.isnan(buf[:, lp * d:]).all())


def test_mask_forms_and_strided_views(dev):
    from evdr_amd import ops
    P, pm, want = small_case(torch.float32)
    Pd, pmd = P.to(dev), pm.to(dev)
    bytes_ = torch.where(pmd, torch.where(torch.arange(33, device=dev)[None] % 2 == 0, 2, 255), 0).to(torch.uint8)
    rows = pmd.t().contiguous().t()
    assert not rows.is_contiguous()
    for name, m in (("uint8", bytes_), ("int64", pmd.long() * 7), ("float32", pmd.float() * 0.5), ("strided", rows)):
        assert_equals_reference(ops.cluster_pages(Pd, m, ls=9, iters=ITERS[-1], return_labels=True), want, f"mask {name}")
    Pt = Pd.transpose(0, 1).contiguous().transpose(0, 1)
    assert not Pt.is_contiguous()
    assert_equals_reference(ops.cluster_pages(Pt, pmd, ls=9, iters=ITERS[-1], return_labels=True), want, "transposed pages")


# ---- 8. streams and the workspace -----------------------------------------------------------------------------------------------------------
def test_two_streams_alternate_shapes_without_a_sync(dev):
    """The workspace belongs to a (device, stream): two streams take a small shape and one with workspace centroids (ls = 313) in turn,
    nothing waits in between, and each stream's workspace grows under its queued launches."""
    from evdr_amd import ops
    shapes = ((33, 9, 64, 4, torch.float32), (700, 313, 32, 3, torch.bfloat16))
    inputs = [tuple(t.to(dev) for t in cc.case(lp, ls, d, dt, n)) for lp, ls, d, n, dt in shapes]
    streams = [torch.cuda.Stream(device=dev) for _ in range(2)]
    torch.cuda.synchronize()
    for s in streams:
        ops._cluster_ws.pop((dev, s.cuda_stream), None)               # a stream of torch's pool may have served an earlier test
    outs = []
    for r in range(6):
        k = (r + r // 2) % 2                                           # stream 0: small, large, small; stream 1: large, small, large
        with torch.cuda.stream(streams[r % 2]):
            outs.append((k, ops.cluster_pages(*inputs[k], ls=shapes[k][1], iters=ITERS[-1], return_labels=True)))
    torch.cuda.synchronize()
    for r, (k, got) in enumerate(outs):
        lp, ls, d, n, dt = shapes[k]
        assert_equals_reference(got, cc.reference(lp, ls, d, dt, n, ITERS[-1])[0], f"launch {r} on stream {r % 2}, shape {k}")


def test_workspace_regrown_between_back_to_back_launches(dev):
    from evdr_amd import ops
    shapes = ((33, 9, 64, 4, torch.float32), (1030, 258, 128, 6, torch.float32), (33, 9, 64, 4, torch.float32))
    inputs = [tuple(t.to(dev) for t in cc.case(lp, ls, d, dt, n)) for lp, ls, d, n, dt in shapes]
    side = torch.cuda.Stream(device=dev)
    torch.cuda.synchronize()
    ops._cluster_ws.pop((dev, side.cuda_stream), None)
    with torch.cuda.stream(side):
        outs = [ops.cluster_pages(*inp, ls=sh[1], iters=ITERS[-1], return_labels=True) for inp, sh in zip(inputs, shapes)]
        sizes = ops._cluster_ws[(dev, side.cuda_stream)].numel()
    torch.cuda.synchronize()
    lib_need = [1030 * 4 * 512, 33 * 4 * 512]
    assert sizes >= lib_need[0] > lib_need[1]
    for r, (got, (lp, ls, d, n, dt)) in enumerate(zip(outs, shapes)):
        assert_equals_reference(got, cc.reference(lp, ls, d, dt, n, ITERS[-1])[0], f"launch {r}")
