"""GPU: the appearance MLP's kernels (csrc/appearance.hip) through
gsplat_hip.appearance_colors, against the torch oracle in fp64 and the
fixture recorded from the reference's module.

The bound is not a number chosen beforehand: HIP's error against the fp64
oracle must be within 4 x the error of the fp32 torch oracle against fp64 for
the same quantity (max-abs for the colours and the per-row gradients,
norm-wise for the gradients summed over rows: the head's tensors and the
embedding rows), with a floor of 1e-6 on the colours.  The margin of 4 is for
a different summation order of the same number of fp32 roundings.  Every
figure is printed before it is asserted (profiles/app_opt/parity.txt is this
file's output under `-s`)."""

import functools

import numpy as np
import pytest
import torch

import app_oracle as O
from conftest import load_golden

pytestmark = pytest.mark.gpu

TILE = 128  # rows of one workgroup pass
SHAPES = ((64, 64), (64,), (64, 64), (64,), (3, 64), (3,))
PER_ROW = ("features", "base_colors", "means")
MARGIN = 4.0
COLOR_FLOOR = 1e-6


def make_inputs(N, C, seed, zero_last=False, dead=False):
    g = torch.Generator().manual_seed(seed)
    inp = dict(features=torch.rand(N, 32, generator=g),
               base_colors=torch.randn(N, 3, generator=g),
               means=torch.randn(N, 3, generator=g),
               campos=torch.randn(C, 3, generator=g) * 3.0,
               embeds=torch.randn(C, 16, generator=g))
    for k, s in zip(O.HEAD_NAMES, SHAPES):  # torch's Linear default, U(+-1/sqrt(64))
        inp[k] = (torch.rand(*s, generator=g) * 2 - 1) * 0.125
    inp["W3"] *= 4.0  # colours that depend on the trunk visibly
    if zero_last:
        inp["W3"].zero_()
        inp["b3"].zero_()
    if dead:  # units that no row switches on, in both layers
        inp["b1"][::3] = -50.0
        inp["b2"][1::4] = -50.0
    v = torch.randn(C, N, 3, generator=g)
    return inp, v


def run_hip(inp, v, deg, masks=None, use_embeds=True):
    import gsplat_hip
    d = {k: t.cuda().requires_grad_(k != "campos") for k, t in inp.items()}
    col = gsplat_hip.appearance_colors(
        d["features"], d["base_colors"], d["embeds"] if use_embeds else None, d["means"],
        d["campos"], [d[k] for k in O.HEAD_NAMES], deg,
        masks=None if masks is None else masks.cuda())
    col.backward(v.cuda())
    grads = {k: d[k].grad.cpu() for k in O.GRAD_NAMES if use_embeds or k != "embeds"}
    return col.detach().cpu(), grads


def check(tag, hip, f32, f64):
    """The rule of the module docstring for (colors, grads) triples."""
    (ch, gh), (c32, g32), (c64, g64) = hip, f32, f64
    e_h = float((ch.double() - c64).abs().max())
    e_r = float((c32.double() - c64).abs().max())
    print(f"{tag} colors: hip {e_h:.3e} fp32 {e_r:.3e}")
    bad = []
    if e_h > max(MARGIN * e_r, COLOR_FLOOR):
        bad.append(("colors", e_h, e_r))
    for k in g64:
        dh, dr = gh[k].double() - g64[k], g32[k].double() - g64[k]
        if k in PER_ROW:
            e_h, e_r, how = float(dh.abs().max()), float(dr.abs().max()), "max"
        else:
            e_h, e_r, how = float(dh.norm()), float(dr.norm()), "l2 "
        print(f"{tag} {k:12s} {how}: hip {e_h:.3e} fp32 {e_r:.3e} (|g|max "
              f"{float(g64[k].abs().max()):.2e})")
        if e_h > MARGIN * e_r:
            bad.append((k, e_h, e_r))
    assert not bad, bad


@functools.lru_cache(maxsize=None)
def oracle(N, C, deg, seed, use_embeds=True, zero_last=False, dead=False, mask_kind=None):
    inp, v = make_inputs(N, C, seed, zero_last, dead)
    masks = make_mask(mask_kind, C, N)
    return (inp, v, masks, O.run(inp, v, deg, torch.float32, masks, use_embeds),
            O.run(inp, v, deg, torch.float64, masks, use_embeds))


def make_mask(kind, C, N):
    if kind is None:
        return None
    g = torch.Generator().manual_seed(5)
    m = torch.rand(C, N, generator=g) > 0.25      # single rows off
    m[:, TILE:2 * TILE] = False                   # a whole workgroup pass off
    m[0, 2 * TILE:2 * TILE + 32] = False          # a whole wave off, one camera
    return m


# N = 1, around one workgroup pass, and three passes with a ragged tail
@pytest.mark.parametrize("N", [1, TILE - 1, TILE, TILE + 1, 3 * TILE + 37])
@pytest.mark.parametrize("C", [1, 2])
def test_parity_sizes(N, C):
    inp, v, _, f32, f64 = oracle(N, C, 3, 11)
    check(f"N={N} C={C} deg=3", run_hip(inp, v, 3), f32, f64)


@pytest.mark.parametrize("deg", [0, 1, 2])
@pytest.mark.parametrize("C", [1, 2])
def test_parity_degrees(deg, C):
    inp, v, _, f32, f64 = oracle(TILE + 37, C, deg, 12)
    check(f"N={TILE + 37} C={C} deg={deg}", run_hip(inp, v, deg), f32, f64)


@pytest.mark.parametrize("C", [1, 2])
def test_parity_without_embeddings(C):
    inp, v, _, f32, f64 = oracle(TILE + 37, C, 3, 13, use_embeds=False)
    hip = run_hip(inp, v, 3, use_embeds=False)
    check(f"N={TILE + 37} C={C} embeds=None", hip, f32, f64)
    # and it is the zero embedding
    zero = dict(inp, embeds=torch.zeros_like(inp["embeds"]))
    col, _ = run_hip(zero, v, 3)
    assert torch.equal(col, hip[0])


def test_parity_masked():
    N, C = 3 * TILE + 37, 2
    inp, v, masks, f32, f64 = oracle(N, C, 3, 14, mask_kind="mixed")
    col, g = run_hip(inp, v, 3, masks=masks)
    check(f"N={N} C={C} masked", (col, g), f32, f64)
    off = ~masks
    assert not col[off].any()
    gone = off.all(0)  # hidden from every camera: no gradient at all
    assert gone.sum() >= TILE
    for k in PER_ROW:
        assert not g[k][gone].any(), k


def test_zero_last_layer_gives_exact_zeros():
    """The trainer starts from a zero last layer: nothing flows back through
    it, and the colours are sigmoid(base_colors)."""
    N, C = TILE + 37, 2
    inp, v, _, f32, f64 = oracle(N, C, 3, 15, zero_last=True)
    col, g = run_hip(inp, v, 3)
    check(f"N={N} C={C} zero last layer", (col, g), f32, f64)
    for k in ("features", "embeds", "means", "W1", "b1", "W2", "b2"):
        assert not g[k].any(), k
    assert g["W3"].any() and g["b3"].any() and g["base_colors"].any()
    want = torch.sigmoid(inp["base_colors"].double())[None].expand(C, -1, -1)
    assert float((col.double() - want).abs().max()) < 1e-7


def test_dead_relu_units():
    N, C = TILE + 37, 2
    inp, v, _, f32, f64 = oracle(N, C, 3, 16, dead=True)
    col, g = run_hip(inp, v, 3)
    check(f"N={N} C={C} dead units", (col, g), f32, f64)
    assert not g["W1"][::3].any() and not g["b1"][::3].any()
    assert not g["W2"][1::4].any() and not g["b2"][1::4].any()
    assert not g["W2"][:, ::3].any()  # nothing comes out of a dead unit
    assert g["W1"][1].any() and g["W2"][0].any()


@pytest.mark.parametrize("tag,C,deg,use", [("c2d3", 2, 3, True), ("c1d1none", 1, 1, False)])
def test_fixture_gradients(tag, C, deg, use):
    """The reference's own module (fp32, CPU) as the fp32 side of the rule."""
    z = load_golden("app_opt")
    inp = {k: torch.from_numpy(z[k]) for k in ("features", "base_colors", "means") + O.HEAD_NAMES}
    inp["campos"] = torch.from_numpy(z["campos"][:C])
    ids = z["embed_ids"][:C]
    inp["embeds"] = torch.from_numpy(z["embeds_table"][ids])
    v = torch.from_numpy(z["v_colors"][:C])
    ref = {k: torch.from_numpy(z[f"{tag}_v_embeds_table"][ids] if k == "embeds"
                               else z[f"{tag}_v_{k}"])
           for k in O.GRAD_NAMES if use or k != "embeds"}
    f32 = (torch.from_numpy(z[f"colors_{tag}"]), ref)
    f64 = O.run(inp, v, deg, torch.float64, use_embeds=use)
    check(f"fixture {tag}", run_hip(inp, v, deg, use_embeds=use), f32, f64)


@pytest.mark.parametrize("C", [1, 2])
@pytest.mark.parametrize("deg", [0, 1, 2, 3])
def test_fixture_colours(C, deg):
    z = load_golden("app_opt")
    import gsplat_hip
    t = lambda k: torch.from_numpy(z[k]).cuda()
    col = gsplat_hip.appearance_colors(
        t("features"), t("base_colors"), t("embeds_table")[t("embed_ids")[:C]], t("means"),
        t("campos")[:C], [t(k) for k in O.HEAD_NAMES], deg)
    err = float((col.cpu() - torch.from_numpy(z[f"colors_c{C}d{deg}"])).abs().max())
    print(f"fixture colours C={C} deg={deg}: {err:.3e}")
    assert err <= COLOR_FLOOR


def test_two_runs_are_bit_identical():
    inp, v, _, _, _ = oracle(3 * TILE + 37, 2, 3, 11)
    (c1, g1), (c2, g2) = run_hip(inp, v, 3), run_hip(inp, v, 3)
    assert torch.equal(c1, c2)
    for k in g1:
        assert torch.equal(g1[k], g2[k]), k


# --------------------------------------------------------- reduce + Adam entry
def _adam_case(C=2, N=3 * TILE + 37, n_img=5):
    from gsplat_hip import appearance as A
    inp, v = make_inputs(N, C, 21)
    g = torch.Generator().manual_seed(22)
    table = torch.randn(n_img, 16, generator=g)
    ids = torch.tensor([3, 1][:C])
    d = {k: t.cuda() for k, t in inp.items()}
    head = [d[k].clone() for k in O.HEAD_NAMES]
    tab, idd = table.cuda(), ids.cuda()
    ws = A.app_workspace(N, C, "cuda")
    A.app_colors_bwd(v.cuda(), d["features"], d["base_colors"], d["means"], d["campos"], head, 3,
                     ws, embeds=tab, embed_ids=idd)
    return A, inp, table, ids, head, tab, idd, ws, N, C


def test_reduce_adam_matches_torch_adam():
    """Adam(lr) on the head and Adam(10 lr, weight_decay) on the whole table,
    two steps from the same gradients, against torch.optim.Adam."""
    A, inp, table, ids, head, tab, idd, ws, N, C = _adam_case()
    lr, wd = 1e-3, 1e-2
    grads = A.app_reduce(ws, N, C).cpu()
    ref_head = [torch.nn.Parameter(inp[k].clone()) for k in O.HEAD_NAMES]
    ref_tab = torch.nn.Parameter(table.clone())
    opts = [torch.optim.Adam(ref_head, lr=lr), torch.optim.Adam([ref_tab], lr=lr * 10,
                                                                weight_decay=wd)]
    m, v2 = torch.zeros(8515, device="cuda"), torch.zeros(8515, device="cuda")
    em, ev = torch.zeros_like(tab), torch.zeros_like(tab)
    gbuf = torch.empty(8515 + 16 * C, device="cuda")
    for step in (1, 2):
        o = 0
        for p in ref_head:
            p.grad = grads[o:o + p.numel()].view_as(p).clone()
            o += p.numel()
        ref_tab.grad = torch.zeros_like(ref_tab)
        for c in range(C):
            ref_tab.grad[ids[c]] += grads[8515 + 16 * c:8515 + 16 * (c + 1)]
        for op in opts:
            op.step()
        A.app_reduce_adam(ws, N, C, gbuf, head, m, v2, lr, step, embeds=tab, embed_ids=idd,
                          embed_exp_avg=em, embed_exp_avg_sq=ev, embed_weight_decay=wd)
    assert torch.equal(gbuf.cpu(), grads)
    for p, q in zip(head, ref_head):
        np.testing.assert_allclose(p.cpu().numpy(), q.detach().numpy(), rtol=2e-6, atol=1e-7)
    np.testing.assert_allclose(tab.cpu().numpy(), ref_tab.detach().numpy(), rtol=2e-6, atol=1e-7)
    # rows no camera shows moved by their weight decay alone
    assert not torch.equal(tab.cpu()[0], table[0])
    st = opts[0].state[ref_head[0]]
    np.testing.assert_allclose(m[:4096].cpu().numpy(), st["exp_avg"].flatten().numpy(),
                               rtol=2e-6, atol=1e-9)


def test_reduce_adam_device_factors_and_skip():
    """The captured step's form: factors from a device buffer give the bits
    of the scalar form; a raised skip flag changes nothing."""
    A, inp, table, ids, head, tab, idd, ws, N, C = _adam_case()
    lr, wd, step = 1e-3, 1e-6, 3
    gbuf = torch.empty(8515 + 16 * C, device="cuda")

    def state():
        return ([h.clone() for h in head], torch.full((8515,), 0.01, device="cuda"),
                torch.full((8515,), 1e-4, device="cuda"), tab.clone(),
                torch.zeros_like(tab), torch.zeros_like(tab))

    a, b, c = state(), state(), state()
    A.app_reduce_adam(ws, N, C, gbuf, a[0], a[1], a[2], lr, step, embeds=a[3], embed_ids=idd,
                      embed_exp_avg=a[4], embed_exp_avg_sq=a[5], embed_weight_decay=wd)
    # the library's host arithmetic: the fp32 arguments in double
    f = lambda x: float(np.float32(x))
    bc1, bc2 = 1.0 - f(0.9) ** step, 1.0 - f(0.999) ** step
    hyper = torch.tensor([f(lr) / bc1, 1.0 / bc2 ** 0.5, f(lr) * f(10.0) / bc1, 0.0],
                         dtype=torch.float64).float().cuda()
    A.app_reduce_adam(ws, N, C, gbuf, b[0], b[1], b[2], 0.0, 0, embeds=b[3], embed_ids=idd,
                      embed_exp_avg=b[4], embed_exp_avg_sq=b[5], embed_weight_decay=wd,
                      hyper=hyper)
    skip = torch.ones(1, dtype=torch.int32, device="cuda")
    before = [t.clone() for t in (*c[0], *c[1:])]
    A.app_reduce_adam(ws, N, C, gbuf, c[0], c[1], c[2], lr, step, embeds=c[3], embed_ids=idd,
                      embed_exp_avg=c[4], embed_exp_avg_sq=c[5], embed_weight_decay=wd,
                      skip=skip)
    for x, y in zip((*a[0], *a[1:]), (*b[0], *b[1:])):
        assert torch.equal(x, y)
    for x, y in zip((*c[0], *c[1:]), before):
        assert torch.equal(x, y)
    assert not torch.equal(a[0][0], head[0])


def test_pieces_replay_as_kernel_nodes_only():
    """The forward, the backward and the reduce + Adam launch captured as a
    HIP graph: four kernel nodes, nothing else; the image is chosen by the
    device index at replay time, and a replay gives the bits of the eager
    launches."""
    from gsplat_hip import appearance as A
    from gsplat_hip.graph_step import check_kernel_nodes_only
    N, C, n_img = 3 * TILE + 37, 1, 5
    inp, v = make_inputs(N, C, 31)
    g = torch.Generator().manual_seed(32)
    d = {k: t.cuda() for k, t in inp.items()}
    vc = v.cuda()
    table0 = torch.randn(n_img, 16, generator=g).cuda()
    ids = torch.zeros(1, dtype=torch.int64, device="cuda")
    hyper = torch.tensor([1e-3, 1.0, 1e-2, 0.0], device="cuda")
    ws = A.app_workspace(N, C, "cuda")

    def fresh():
        return ([d[k].clone() for k in O.HEAD_NAMES], torch.zeros(8515, device="cuda"),
                torch.zeros(8515, device="cuda"), table0.clone(), torch.zeros_like(table0),
                torch.zeros_like(table0), torch.empty(C, N, 3, device="cuda"),
                torch.empty(N, 3, device="cuda"), torch.empty(N, 32, device="cuda"),
                torch.empty(N, 3, device="cuda"), torch.empty(8515 + 16 * C, device="cuda"))

    def body(s):
        head, m, v2, tab, em, ev, col, vb, vf, vm, gbuf = s
        A.app_colors_fwd(d["features"], d["base_colors"], d["means"], d["campos"], head, 3,
                         embeds=tab, embed_ids=ids, out=col)
        A.app_colors_bwd(vc, d["features"], d["base_colors"], d["means"], d["campos"], head, 3,
                         ws, embeds=tab, embed_ids=ids, v_base_colors=vb, v_features=vf,
                         v_means=vm)
        A.app_reduce_adam(ws, N, C, gbuf, head, m, v2, 0.0, 0, embeds=tab, embed_ids=ids,
                          embed_exp_avg=em, embed_exp_avg_sq=ev, embed_weight_decay=1e-6,
                          hyper=hyper)

    eager, cap = fresh(), fresh()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        body(fresh())  # warm-up outside the capture
    torch.cuda.current_stream().wait_stream(side)
    graph = torch.cuda.CUDAGraph(keep_graph=True)
    with torch.cuda.graph(graph, capture_error_mode="thread_local"):
        body(cap)
    census = check_kernel_nodes_only(graph)
    assert census.get("kernel") == 4, census
    graph.instantiate()
    for image in (3, 1):
        ids.fill_(image)
        body(eager)
        graph.replay()
        torch.cuda.synchronize()
        for x, y in zip((*eager[0], *eager[1:]), (*cap[0], *cap[1:])):
            assert torch.equal(x, y)
