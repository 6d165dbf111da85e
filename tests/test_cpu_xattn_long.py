"""Long prompts on the CPU: the blocked cross-attention arithmetic against fp64 (tests/xattn_long_ref.py), the selection of the long form
(sdxl_debug_igemm_select), and the 77-token chunking of the tokenizer.

The arithmetic checks show, without a GPU, that the inputs tests/test_gpu_xattn_long.py uses (a) leave the kernel room -- the clean emulation of its
roundings stays below half of the bound TOL_F16 at every shape -- and (b) expose every defect the blocked form invites at least ten times outside that
bound.  Which shapes can expose which defect is a matter of the shape: a mask that ignores the block offset is invisible where nothing is masked
(192, 384 keys) or where the padding keys' weight is small next to a dominant key; so the requirement per defect is on the worst case over the GPU
test's cases, and the table of all ratios is printed (recorded in profiles/long_context_xattn_tests.txt)."""
import ctypes
import gzip
import importlib
import os

import pytest
import torch

import select_cases as sc
import xattn_long_ref as XR
from util import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOKENIZER_GOLDEN = os.path.join(ROOT, "tests", "golden", "tokenizer")


# ------------------------------------------------------------------ arithmetic
def _cases():
    for i, (B, Nq, Nk, C, _) in enumerate(XR.SHAPES):
        yield (B, Nq, Nk, C), dict(rot=i)
    B, Nq, Nk, C, _ = XR.UNDERFLOW
    yield (B, Nq, Nk, C), dict(kinds=["last"] * B, factor=8.0)


@pytest.fixture(scope="module")
def ratios():
    """per case: error / TOL_F16 of the clean emulation and of every planted defect, computed once"""
    rows = []
    for shape, kw in _cases():
        x, gamma, beta, wq, k, v = XR.inputs(*shape, **kw)
        q = XR.query_fp64(x, gamma, beta, wq)
        ref = XR.attention_fp64(q, k, v)
        row = {"shape": shape, "kw": kw, "clean": rel_err(XR.emulate(q, k.double(), v.double()), ref) / XR.TOL_F16}
        assert torch.isfinite(ref).all()
        for d in XR.DEFECTS:
            out = XR.emulate(q, k.double(), v.double(), d)
            row[d] = rel_err(torch.nan_to_num(out, nan=1e30, posinf=1e30, neginf=-1e30), ref) / XR.TOL_F16
        rows.append(row)
        print("xattn_long emulation %-24s %-28s clean %.3f  " % (shape, kw, row["clean"]) + "  ".join("%s %.1f" % (d, row[d]) for d in XR.DEFECTS))
    return rows


def test_clean_emulation_leaves_the_kernel_room(ratios):
    for r in ratios:
        assert r["clean"] < 0.5, r


@pytest.mark.parametrize("defect", XR.DEFECTS)
def test_planted_defect_is_far_outside_the_bound(ratios, defect):
    worst = max(r[defect] for r in ratios)
    assert worst >= 10.0, (defect, [(r["shape"], r[defect]) for r in ratios])


def test_underflow_case_is_finite(ratios):
    r = ratios[-1]
    assert r["kw"].get("factor") == 8.0 and r["clean"] < 0.5


# ------------------------------------------------------------------ selection
@pytest.fixture(scope="module")
def lib(pkg):
    if not os.path.exists(pkg.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    l = ctypes.CDLL(pkg.LIB_PATH)
    l.sdxl_debug_igemm_select.restype = ctypes.c_int
    l.sdxl_last_error.restype = ctypes.c_char_p
    return l


def _select(lib, xa_nctx, N=1280, rows=1024, **knobs):
    """the step's fused query projection (CFG pair at the 32^2 level: M = 2 x 1024, N = K = 1280, folded LayerNorm, fragment-order weights)"""
    case = dict(batch=2, rows_per_entry=rows, N=N, cin=N, ksize=1, stride=1, up=0, act=0, n_split=-1, a_dt=sc.F16, c_dt=sc.F16, compute_dt=sc.F16,
                xa_nctx=xa_nctx, shadow_lo_sign=0, present=sc.SPLITK_WS | sc.XA_K | sc.LN_STAT | sc.WF, misaligned=0)
    out = sc.IgemmChoice()
    status = lib.sdxl_debug_igemm_select(ctypes.byref(sc.IgemmCase(**case)), ctypes.byref(sc.Knobs(**dict(sc.DEFAULT_KNOBS, **knobs))), ctypes.byref(out))
    return status, out, lib.sdxl_last_error().decode() if status else ""


@pytest.mark.parametrize("xa_nctx,blocks", [(77, 1), (96, 1), (97, 2), (154, 2), (231, 3), (384, 4)])
def test_long_contexts_select_the_weights_in_registers_form(lib, xa_nctx, blocks):
    status, out, msg = _select(lib, xa_nctx)
    assert status == 0, msg
    assert (out.family, out.wreg_xattn_selected, out.xa) == (4, 1, blocks)
    short = _select(lib, 77)[1]
    assert (out.bm, out.bn, out.ns, out.grid, out.block, out.lds) == (short.bm, short.bn, short.ns, short.grid, short.block, short.lds)


def test_beyond_the_limit_is_refused_like_before(lib):
    status, _, msg = _select(lib, 385)
    assert status != 0 and "fused cross-attention needs a plain f16 projection" in msg      # the text 97 keys were refused with before


@pytest.mark.parametrize("N,knobs", [(320, {}), (192, {}), (1280, dict(wreg_xattn=0)), (1280, dict(igemm_wreg=0)), (1280, dict(igemm_variant=45))])
def test_long_context_without_the_weights_in_registers_form_is_refused(lib, N, knobs):
    """N % 128 != 0, the A/B knobs, a forced pipe tile: the pipe epilogues hold one 96-key block -- never a pipe kernel with more keys"""
    status, out, _ = _select(lib, 154, N=N, **knobs)
    assert status != 0
    status, out, msg = _select(lib, 77, N=N, **knobs)
    assert status == 0 and out.xa == 1, msg


def test_long_form_does_not_depend_on_the_batch(lib):
    picks = set()
    for batch in (1, 2, 3, 4, 8):
        case = dict(batch=batch, rows_per_entry=1024, N=1280, cin=1280, ksize=1, stride=1, up=0, act=0, n_split=-1, a_dt=sc.F16, c_dt=sc.F16,
                    compute_dt=sc.F16, xa_nctx=154, shadow_lo_sign=0, present=sc.SPLITK_WS | sc.XA_K | sc.LN_STAT | sc.WF, misaligned=0)
        out = sc.IgemmChoice()
        assert lib.sdxl_debug_igemm_select(ctypes.byref(sc.IgemmCase(**case)), ctypes.byref(sc.Knobs(**sc.DEFAULT_KNOBS)), ctypes.byref(out)) == 0
        picks.add((out.family, out.xa, out.wreg_xattn_selected))
    assert picks == {(4, 2, 1)}


# ------------------------------------------------------------------ tokenizer
@pytest.fixture(scope="module")
def tokdir(tmp_path_factory):
    """the tokenizer assets, unpacked from the gzipped copies under tests/golden/tokenizer/ (as tests/test_cpu_oracle_and_abi.py does)"""
    d = tmp_path_factory.mktemp("tokenizer")
    for rel in ("clip/bpe_simple_vocab_16e6.txt", "open_clip/merges.txt", "open_clip/vocab.txt"):
        (d / rel).parent.mkdir(parents=True, exist_ok=True)
        with gzip.open(os.path.join(TOKENIZER_GOLDEN, rel + ".gz"), "rb") as fh:
            (d / rel).write_bytes(fh.read())
    return str(d)


@pytest.fixture(scope="module")
def tok(pkg):
    return importlib.import_module(pkg.__name__ + ".tokenizer")


_WORDS = "a photograph of an astronaut riding a horse on the moon at sunset with dramatic lighting and long shadows over grey dust".split()


def _prompt(t, n_tokens):
    """a prompt of exactly n_tokens ids (without sot / eot)"""
    words, i = [], 0
    while len(t.encode(" ".join(words), False, False)) < n_tokens:
        words.append(_WORDS[i % len(_WORDS)])
        i += 1
    text = " ".join(words)
    assert len(t.encode(text, False, False)) == n_tokens, "every word of the list is one token"
    return text


@pytest.mark.parametrize("which", ["ClipTokenizer", "OpenClipTokenizer"])
@pytest.mark.parametrize("n_tokens,chunks", [(10, 1), (75, 1), (76, 2), (200, 3)])
def test_prompts_are_cut_into_77_token_chunks(tok, tokdir, which, n_tokens, chunks):
    t = getattr(tok, which)(tokdir)
    text = _prompt(t, n_tokens)
    plain = t.encode(text, False, False)
    got = tok.tokenize_text_chunks(text, t, 77, 4)
    assert len(got) == chunks
    pieces = []
    for i, ch in enumerate(got):
        n = min(75, n_tokens - 75 * i)
        assert len(ch) == 77 and ch[0] == tok.SOT and ch[1 + n] == tok.EOT
        assert ch[2 + n:] == [t.padding_token()] * (75 - n)
        pieces += ch[1:1 + n]
    assert pieces == plain
    assert tok.tokenize_text_chunks(text, t, 77, 1) == [tok.tokenize_text(text, t, 77)]
    # text beyond max_chunks chunks is dropped, whole chunks stay as they are
    assert tok.tokenize_text_chunks(text, t, 77, 2) == got[:2]


def test_empty_prompt_is_one_chunk(tok, tokdir):
    t = tok.OpenClipTokenizer(tokdir)
    assert tok.tokenize_text_chunks("", t, 77, 4) == [tok.tokenize_text("", t, 77)]
    with pytest.raises(ValueError):
        tok.tokenize_text_chunks("a", t, 77, 0)
