"""The entries of the UNet's block plan one by one (sdxl_unet_block -> UNet::run_block -> run_entry: the code UNet::forward runs, with forward's row
strides, concat-slice offsets, emb_off slices and cross-attention cache offsets) against fp64 at SDXL widths: the base configuration with the deepest
level's transformer depth cut to 2, seeded synthetic weights, B = 2, 77 context tokens.  Cases, references, emulations and bounds come from
tests/unet_block_ref.py (bound = margin x the error of the mode's CPU emulation on the same operands, never a GPU result);
tests/test_cpu_unet_block_ref.py shows that the planted defects leave those bounds.

The same tests over the refiner configuration (transformer depths cut to 2; R.RF_CASES: 12 / 24 heads, eight-slice split-K on whole, ragged and 64-row
tiles, ResU entries with either upsample form, K up to 27648) stand at the end of the file: the base handles are released before the first refiner
handle is made.  A refiner handle's arena is printed next to its creation time; the six hold 30.7 GiB together (3.5 ... 6.6 GiB each) and stay alive to
the end of the module, case-major like the base runs.  Above REFINER_HANDLE_BYTES together the runs would have to be ordered dtype-major with one
handle alive at a time: _unet asserts the sum.

Every assertion prints error / bound / ratio first (pytest -s; recorded in profiles/unet_block_tests.txt and profiles/refiner_block_tests.txt)."""
import ctypes
import time

import pytest
import torch

import unet_block_ref as R
from oracle import config as OC
from util import to_pkg_cfg, unet_weights

pytestmark = pytest.mark.gpu

RUNS = [(c[0], dt) for c in R.CASES for dt in R.case_dtypes(c[0])]
RF_RUNS = [(c[0], dt) for c in R.RF_CASES for dt in R.case_dtypes(c[0])]
REFINER_HANDLE_BYTES = 64 << 30      # what the six refiner handles may hold together on a shared machine


@pytest.fixture(scope="module")
def handles():
    """one handle per (configuration, dtype) for the whole module (created on first use, released with the module)"""
    d = {}
    yield d
    d.clear()


def _unet(pkg, ctx, handles, dtype, model="base"):
    if (model, dtype) not in handles:
        if model == "refiner":      # the base handles go before the first refiner handle is made
            for k in [k for k in handles if k[0] != "refiner"]:
                del handles[k]
        t0 = time.perf_counter()
        u = pkg.UNet(ctx, to_pkg_cfg(pkg, R.CONFIGS[model]), dtype, seed=pkg.SEED_F16_WEIGHTS if R.mode_of(dtype).f16w else 0)
        torch.cuda.synchronize()
        if model == "base":
            print(f"unet_block handle dtype {dtype}: created in {time.perf_counter() - t0:.2f} s")
        else:
            print(f"unet_block refiner handle dtype {dtype}: created in {time.perf_counter() - t0:.2f} s, weight arena {u.weight_arena()[1] / 2 ** 30:.2f} GiB")
        assert u.mix_classes() == R.MIX_EXPECTED.get(dtype, 0), "the mode fell back to other classes"      # (mix_of: the bits do not depend on the configuration)
        handles[(model, dtype)] = u
        held = sum(h.weight_arena()[1] for k, h in handles.items() if k[0] == "refiner")
        assert held <= REFINER_HANDLE_BYTES, f"the refiner handles hold {held / 2 ** 30:.1f} GiB together: run dtype-major, one alive at a time"
    return handles[(model, dtype)]


def _run(u, name, entries=slice(None)):
    _, section, index, _, _, _ = R.case(name)
    x, emb, context = (t[entries].contiguous().cuda() for t in R.inputs(name))
    return u.run_block(section, index, x, emb, context)


def _check_bound(out, name, dtype, what=""):
    errs = R.errors(out.cpu(), name, f16w=R.mode_of(dtype).f16w)
    bnd, emu = R.bounds(name, dtype)
    for b in range(len(errs)):
        print(f"unet_block {name}{what} dtype {dtype} entry {b}: error {errs[b]:.3e}  bound {bnd[b]:.3e} "
              f"({R.mode_of(dtype).margin:g} x emulation {emu[b]:.3e})  ratio {errs[b] / bnd[b]:.3f}")
    assert all(e <= b for e, b in zip(errs, bnd)), (name, dtype, errs, bnd)


@pytest.mark.parametrize("name,dtype", RUNS)
def test_block_within_emulation_bound(pkg, ctx, handles, name, dtype):
    _within_emulation_bound(pkg, ctx, handles, name, dtype)


def _within_emulation_bound(pkg, ctx, handles, name, dtype):
    out = _run(_unet(pkg, ctx, handles, dtype, R.CONFIG_OF[name]), name)
    assert tuple(out.shape) == tuple(R.ref64(name, f16w=R.mode_of(dtype).f16w).shape)
    _check_bound(out, name, dtype)


@pytest.mark.parametrize("name,dtype", [(n, dt) for n in ("rest_640_skip", "rest_1280", "rest_1280_bucket") for dt in R.case_dtypes(n)])
def test_block_entries_are_independent(pkg, ctx, handles, name, dtype):
    if name == "rest_640_skip" and dtype == 3:
        name = "rest_640_skip_mag"      # one operand scale per entry: entry 1 (2^10 x) next to entry 0 gets the bits it gets alone
    _entries_are_independent(pkg, ctx, handles, name, dtype)


def _entries_are_independent(pkg, ctx, handles, name, dtype):
    u = _unet(pkg, ctx, handles, dtype, R.CONFIG_OF[name])
    pair, alone = _run(u, name), _run(u, name, slice(1, 2))
    assert torch.equal(pair[1:2], alone), f"{name} dtype {dtype}: entry 1 alone differs from entry 1 inside the pair by {(pair[1:2] - alone).abs().max().item():.3e}"


@pytest.mark.parametrize("dtype", [0, 1, 2, 3, 5, 7])
def test_block_keeps_no_state_between_calls(pkg, ctx, handles, dtype):
    # ping-pong statistics buffers, tickets, split-K counters and the zero-filled V^T are per call: another entry at another size in between changes nothing
    _keeps_no_state(_unet(pkg, ctx, handles, dtype), "rest_1280_bucket", "rest_640_skip")


def _keeps_no_state(u, a, b):
    first = _run(u, a)
    other = _run(u, b)
    assert torch.equal(first, _run(u, a))
    assert torch.equal(other, _run(u, b))
    assert torch.equal(first, _run(u, a))


@pytest.mark.parametrize("option,dtype", [("set_gn_from_producer", 1), ("set_gn_from_producer", 2), ("set_fused_cross_attention", 1), ("set_fused_cross_attention", 5)])
def test_block_kernel_paths(pkg, ctx, handles, option, dtype):
    _kernel_paths(_unet(pkg, ctx, handles, dtype), "rest_1280", option, dtype)


def _kernel_paths(u, name, option, dtype):
    try:
        for on in (False, True):
            getattr(u, option)(on)
            out = _run(u, name)
            _check_bound(out, name, dtype, f" {option}({on})")
            assert torch.equal(out, _run(u, name)), f"{option}({on}): the replay differs"
    finally:
        getattr(u, option)(True)


@pytest.mark.parametrize("dtype,model", [pytest.param(dt, m, id=pre + str(dt)) for m, pre in (("tiny", ""), ("tiny_refiner", "refiner-")) for dt in (0, 1, 3, 7)])
def test_chained_blocks_reproduce_forward(pkg, ctx, dtype, model):
    # run_block over the whole plan of the tiny model, the skip concatenations on this side: the bits of forward -- the entry runs forward's code with
    # forward's strides.  emb through the kernels forward's embedding chain launches (timestep_embedding, gemv).  The tiny refiner: the four-level plan
    # with ResU entries, a deepest level of ResBlocks alone and y of its own width.
    ocfg = OC.tiny_config() if model == "tiny" else OC.tiny_refiner_config()
    f16w = dtype == 7
    W = {k: (v.half().float() if f16w and not k.endswith(".eps") else v).cuda() for k, v in unet_weights(ocfg).items()}
    u = pkg.UNet(ctx, to_pkg_cfg(pkg, ocfg), dtype, seed=pkg.SEED_F16_WEIGHTS if f16w else 0)
    x = torch.from_numpy(OC.arb_tensor(2, 4, 16, 16)).cuda()
    context = torch.from_numpy(OC.arb_tensor(2, 5, ocfg.context_dim)).cuda()
    y = torch.from_numpy(OC.arb_tensor(2, ocfg.adm_in_channels)).cuda()
    t = torch.tensor([999, 1], dtype=torch.int32).cuda()
    ref = u.forward(x, t, context, y)
    gd = 1 if dtype == 1 else 0 if dtype == 0 else 3      # the GEMV weights of a split-operand model are packed fp32
    lin = lambda v, n, **kw: pkg.gemv(ctx, v, W[n + ".weight"], W[n + ".bias"], dtype=gd, **kw)      # noqa: E731
    l_emb = lin(lin(y, "lin1_label_embed", silu_out=True), "lin2_label_embed")
    emb = lin(lin(pkg.timestep_embedding(ctx, t.float(), ocfg.model_channels), "lin1_time_embed", silu_out=True), "lin2_time_embed", yadd=l_emb)
    inp, _, out = OC.unet_block_plan(ocfg)
    h, saved = x, []
    for i in range(len(inp)):
        h = u.run_block("input", i, h, emb, context)
        saved.append(h)
    h = u.run_block("middle", 0, h, emb, context)
    for j in range(len(out)):
        h = u.run_block("output", j, torch.cat([h, saved.pop()], dim=1), emb, context)
    eps = u.run_block("head", 0, h, emb, context)
    assert eps.shape == ref.shape
    assert torch.equal(eps, ref), f"dtype {dtype}: the chained entries differ from forward by {(eps - ref).abs().max().item():.3e}"
    # run_block replaced the context and left no label embedding: nothing steps on it until the conditioning is set again
    with pytest.raises(pkg.EngineError, match="set_context must be called again"):
        u.eager_forward_ms(2, 16, 16)
    assert torch.equal(u.forward(x, t, context, y), ref), "forward after run_block differs"
    assert u.eager_forward_ms(2, 16, 16) > 0.0


def test_block_refuses_bad_arguments(pkg, ctx, handles):
    u = _unet(pkg, ctx, handles, 0)
    x, emb, context = (t.cuda() for t in R.inputs("res_320"))
    good = u.run_block("input", 1, x, emb, context)
    n_in = len(OC.unet_block_plan(R.CFG)[0])
    for bad in (lambda: u.run_block("input", n_in, x, emb, context),                    # index outside the plan
                lambda: u.run_block("output", -1, x, emb, context),
                lambda: u.run_block("middle", 1, x, emb, context),
                lambda: u.run_block("tail", 0, x, emb, context),
                lambda: u.run_block("input", 4, torch.cat([x, x], 1), emb, context),  # 640 channels into 320 -> 640
                lambda: u.run_block("input", 1, x[:, :, :6, :6], emb, context),         # level 0 at 6 x 6: no forward has it (24 / 4 levels)
                lambda: u.run_block("input", 4, x[:, :, :3, :3], emb, context),         # level 1 at 3 x 3: a 6 x 6 forward
                lambda: u.run_block("input", 1, x, emb[:1], context),                   # one entry's emb for two
                lambda: u.run_block("input", 8, torch.zeros(1, 1280, 128, 128, device="cuda"), emb[:1], context[:1]),   # level 2 at 128 x 128: a 512 x 512 plan
                lambda: u.run_block("input", 1, x, None, context),                      # null tensors (refused by the binding; the engine's own refusal: below)
                lambda: u.run_block("input", 1, x, emb, None),
                lambda: u.run_block("input", 1, None, emb, context)):
        with pytest.raises(pkg.EngineError):
            bad()
    # the entry itself, past the binding's guards: every refusal is SDXL_ERR_INVALID (1) before anything is launched
    out, shape = torch.empty_like(good), (ctypes.c_int64 * 4)()
    p = lambda t: ctypes.c_void_p(None if t is None else t.data_ptr())      # noqa: E731

    def raw(section=0, index=1, xx=x, ee=emb, cc=context, B=2, c_in=320, h=16, w=16, n_ctx=R.N_CTX, oo=out, handle=u.h):
        return pkg.lib().sdxl_unet_block(handle, None, section, index, p(xx), p(ee), p(cc), B, c_in, h, w, n_ctx, p(oo), shape)
    assert raw(oo=None) == 0 and tuple(shape) == tuple(good.shape)      # the shape query launches nothing
    for kw in (dict(xx=None), dict(ee=None), dict(cc=None), dict(section=4), dict(section=-1), dict(index=n_in), dict(B=0), dict(B=9), dict(c_in=321),
               dict(h=0), dict(h=6, w=6), dict(n_ctx=0), dict(handle=None),
               dict(section=0, index=8, c_in=1280, h=65, w=64, oo=None), dict(section=0, index=8, c_in=1280, h=128, w=128, oo=None),   # 260 x 256, 512 x 512 plans
               dict(h=257, w=16, oo=None)):
        assert raw(**kw) == 1, (kw, pkg.lib().sdxl_last_error().decode())
    assert raw() == 0 and torch.equal(out, good)
    assert torch.equal(u.run_block("input", 1, x, emb, context), good), "the handle is not usable after a refused call"


# ------------------------------------------------------------------------------------------------------------------ the refiner configuration
@pytest.mark.parametrize("name,dtype", RF_RUNS)
def test_refiner_block_within_emulation_bound(pkg, ctx, handles, name, dtype):
    _within_emulation_bound(pkg, ctx, handles, name, dtype)


@pytest.mark.parametrize("name,dtype", [(n, dt) for n in ("rf_rest_768_skip", "rf_rest_1536_bucket", "rf_res_1536_deep_bucket", "rf_out_3072_up_bucket")
                                        for dt in R.case_dtypes(n)])
def test_refiner_block_entries_are_independent(pkg, ctx, handles, name, dtype):
    # the two 18 x 14 cases: 252 rows per entry, so the second 256-row tile of the pair holds rows of both entries and goes through the eight-slice
    # counters and workspace; alone, entry 1 starts a tile
    if name == "rf_rest_768_skip" and dtype == 3:
        name = "rf_rest_768_skip_mag"
    _entries_are_independent(pkg, ctx, handles, name, dtype)


@pytest.mark.parametrize("dtype", [0, 1, 2, 3, 5, 7])
def test_refiner_block_keeps_no_state_between_calls(pkg, ctx, handles, dtype):
    _keeps_no_state(_unet(pkg, ctx, handles, dtype, "refiner"), "rf_middle_1536_bucket", "rf_rest_768_skip")


@pytest.mark.parametrize("option,dtype", [("set_gn_from_producer", 1), ("set_gn_from_producer", 2), ("set_fused_cross_attention", 1), ("set_fused_cross_attention", 5)])
def test_refiner_block_kernel_paths(pkg, ctx, handles, option, dtype):
    _kernel_paths(_unet(pkg, ctx, handles, dtype, "refiner"), "rf_rest_1536", option, dtype)
