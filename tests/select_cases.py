"""Deterministic case lists of the kernel-selection table (tests/golden/select_table.npz) and the ctypes mirror of the two
debug entries.  The table's entries are in the order these generators yield.

How the table was made (never from csrc/select.cpp): in a copy of the commit BEFORE the selection moved into select.cpp, the bodies of
the launch templates -- launch_glds, launch_pipe, launch_wide, launch_wreg_t, launch_cfg and the hipLaunchKernelGGL sites of
launch_attention_d64 -- were replaced by a recorder of their template arguments, grid, block, LDS bytes and splitk, the device
lookups (current device, zero page) by stubs, and the four translation units compiled host-only; two entries with the signatures of
sdxl_debug_igemm_select / sdxl_debug_attn_select set the old knob setters, built the parameter block with csrc/select_debug.h, called
launch_igemm / launch_attention_d64 and the three old predicates, and `run()` below drove them.  Columns the old templates had no
argument for are facts of the kernels that the recorder wrote as constants: wgm / nw of the 4-wave (2 x 2) GLDS and generic kernels,
ns = 2 of the generic kernel's double buffer, nw = 8 of the wide and weights-in-registers kernels.  Release library only: the
measure-only twins are not in the table.

The issue's cross product is kept whole where the selection can depend on an axis and reduced where it cannot be afforded (the
full product of all axes is ~10^7 cases):
  * rows x batch x WIDTHS x the 8 geometries x every operand form x Wf, default knobs: complete; the same with misaligned operands;
  * every forced release number (and -1): all rows, batches and geometries; numbers > 0 over the f16 forms only (the number is read
    for f16 compute alone), Wf on the linear geometry only (the one geometry whose selection reads it);
  * the other knobs, a missing zero page and warming workgroups: the CFG pair (batch 2), geometries (1,1,0) and (3,1,0) -- these
    switch a rule on or off as a whole, and the batch-independence of each rule is covered by the default-knob product;
  * N x K: 16 (N, cin) pairs the models have instead of the product of the two lists, chosen so that with ksize 1 and 3 K takes
    320 ... 27648 incl. 10240 (exactly 160 k-tiles), 5760 / 11520 and N takes both sides of 1536.
The fixture stores the distinct result rows once and an index per case (integers only)."""
from __future__ import annotations

import ctypes
import itertools

import numpy as np

F32, F16, HL = 0, 1, 2
WF, R, EBIAS, STAT_OUT, LN_STAT, GN_PART, SHADOW, XA_K, XA_K_LO, ACC_SCALE, SPLITK_WS, XSPLIT_WS, MASK, WARM = (1 << i for i in range(14))

KNOB_NAMES = ("igemm_variant", "igemm_wreg", "wreg_xattn", "hl_tile96", "igemm_tsw", "igemm_unrolled", "wide_db", "attn_variant", "attn_xsplit", "zero_page")
DEFAULT_KNOBS = dict(igemm_variant=0, igemm_wreg=1, wreg_xattn=1, hl_tile96=29, igemm_tsw=1, igemm_unrolled=1, wide_db=0, attn_variant=0, attn_xsplit=1, zero_page=1)
IGEMM_CASE_FIELDS = ("batch", "rows_per_entry", "N", "cin", "ksize", "stride", "up", "act", "n_split", "a_dt", "c_dt", "compute_dt", "xa_nctx",
                     "shadow_lo_sign", "present", "misaligned")
IGEMM_CHOICE_FIELDS = ("family", "bm", "bn", "ns", "wgm", "nw", "elem", "a_elem", "xa", "xh", "tsw", "s2", "splitk", "mode", "db", "measure", "grid",
                       "block", "lds", "gn_part_ok", "wreg_selected", "wreg_xattn_selected")
ATTN_CASE_FIELDS = ("B", "H", "Nq", "Nk", "dt", "present", "misaligned")
ATTN_CHOICE_FIELDS = ("kernel", "mix", "big_heads", "ns", "elem", "ko", "grid_x", "grid_y", "block", "lds")


def _struct(name, fields, unsigned=("present",)):
    return type(name, (ctypes.Structure,), {"_fields_": [(f, ctypes.c_uint if f in unsigned else ctypes.c_int) for f in fields]})


Knobs = _struct("Knobs", KNOB_NAMES)
IgemmCase = _struct("IgemmCase", IGEMM_CASE_FIELDS)
IgemmChoice = _struct("IgemmChoice", IGEMM_CHOICE_FIELDS)
AttnCase = _struct("AttnCase", ATTN_CASE_FIELDS)
AttnChoice = _struct("AttnChoice", ATTN_CHOICE_FIELDS)

ROWS = (64, 256, 1024, 4096, 16384)
BATCHES = (1, 2, 3, 4, 8)
# (N, cin): channel widths of SDXL base, refiner and VAE; with ksize 3 the K values 2880 ... 27648 straddle the 160 k-tile split-K
# bar (K = 10240), the N values its N <= 1536 bar
WIDTHS = ((320, 320), (640, 320), (640, 640), (640, 1920), (1280, 640), (1280, 1280), (1280, 2560), (1280, 5120), (1536, 1536), (1536, 3072),
          (3840, 1280), (3840, 3072), (10240, 1280), (1280, 10240), (512, 512), (320, 4))
GEOMETRIES = tuple(itertools.product((1, 3), (1, 2), (0, 1)))      # ksize, stride, up
# forced release variant numbers (sdxl_debug_set "igemm_variant") next to 0 = auto
FORCED = (-1, 4, 6, 26, 35, 36, 38, 44, 45, 46, 47, 49, 60, 62)


def _forms(N):
    """operand-presence forms the engine produces: (compute_dt, a_dt, c_dt, act, n_split, present, shadow_lo_sign, linear_only)"""
    qkv = N * 2 // 3 if N % 3 == 0 else N // 2
    ws = SPLITK_WS
    return (
        (F16, F16, F16, 0, -1, ws, 0, False), (F16, F16, F16, 0, -1, ws | R, 0, False), (F16, F16, F16, 0, -1, ws | EBIAS, 0, False),
        (F16, F16, F16, 0, -1, ws | GN_PART, 0, False), (F16, F16, F16, 0, -1, ws | GN_PART | EBIAS, 0, False), (F16, F16, F16, 0, -1, 0, 0, False),
        (F16, F32, F16, 0, -1, ws, 0, False),
        (F16, F16, F16, 1, -1, ws | LN_STAT, 0, True), (F16, F16, F16, 1, -1, ws, 0, True),                      # GEGLU
        (F16, F16, F16, 0, qkv, ws | LN_STAT, 0, True), (F16, F16, F16, 0, qkv, ws, 0, True),                     # fused QKV
        (F16, F16, F16, 0, -1, ws | LN_STAT, 0, True), (F16, F16, F16, 0, -1, ws | STAT_OUT | R, 0, True),
        (F16, F16, F32, 0, -1, ws | R, 0, True),
        (F16, F16, F32, 0, -1, ws | R | STAT_OUT | SHADOW, 0, True), (F16, F16, F32, 0, -1, ws | R | STAT_OUT | SHADOW, 1, True),
        (F16, F16, F32, 0, -1, ws | R | STAT_OUT | SHADOW, -1, True),
        (F16, F16, F16, 0, -1, ws | XA_K, 0, True), (F16, F16, F16, 0, -1, ws | XA_K | LN_STAT, 0, True),
        (F16, F16, HL, 0, -1, ws | XA_K | XA_K_LO, 0, True), (F16, F16, F16, 0, -1, ws | XA_K | R, 0, True),
        (F32, F32, F32, 0, -1, ws, 0, False), (F32, F32, F32, 0, -1, ws | EBIAS | R, 0, False), (F32, F32, F32, 1, -1, ws, 0, True),
        (F32, F32, F32, 0, qkv, ws, 0, True),
        (HL, HL, F32, 0, -1, ws | ACC_SCALE, 0, False), (HL, HL, F32, 0, -1, ws | ACC_SCALE | EBIAS | R, 0, False),
        (HL, HL, F32, 0, -1, ws | ACC_SCALE | GN_PART, 0, False), (HL, HL, HL, 0, -1, ws | ACC_SCALE, 0, True), (HL, HL, HL, 1, -1, ws | ACC_SCALE, 0, True),
        (HL, HL, HL, 0, qkv, ws | ACC_SCALE, 0, True), (HL, HL, F32, 0, -1, ACC_SCALE, 0, False),
    )


def _shape_cases(batches, geometries, f16_only=False, wf_everywhere=True):
    for (N, cin), rows, batch, (ksize, stride, up) in itertools.product(WIDTHS, ROWS, batches, geometries):
        linear = (ksize, stride, up) == (1, 1, 0)
        for cdt, adt, odt, act, n_split, present, lo, linear_only in _forms(N):
            if (linear_only and not linear) or (f16_only and cdt != F16):
                continue
            for wf in ((0, WF) if cdt == F16 and (linear or wf_everywhere) else (0,)):
                yield dict(batch=batch, rows_per_entry=rows, N=N, cin=cin, ksize=ksize, stride=stride, up=up, act=act, n_split=n_split, a_dt=adt, c_dt=odt,
                           compute_dt=cdt, xa_nctx=77, shadow_lo_sign=lo, present=present | wf, misaligned=0)


def igemm_cases():
    """(case, knobs) pairs; see the module docstring for what is complete and what is reduced"""
    for c in _shape_cases(BATCHES, GEOMETRIES):
        yield c, dict(DEFAULT_KNOBS)
    for c in _shape_cases(BATCHES, GEOMETRIES):
        yield dict(c, misaligned=1), dict(DEFAULT_KNOBS)
    for v in FORCED:
        for c in _shape_cases(BATCHES, GEOMETRIES, f16_only=v > 0, wf_everywhere=False):
            yield c, dict(DEFAULT_KNOBS, igemm_variant=v)
    pair = list(_shape_cases((2,), ((1, 1, 0), (3, 1, 0))))
    for over in (dict(igemm_wreg=0), dict(wreg_xattn=0), dict(igemm_tsw=0), dict(zero_page=0), dict(hl_tile96=0), dict(hl_tile96=1), dict(hl_tile96=2 | 1),
                 dict(hl_tile96=4), dict(hl_tile96=8), dict(hl_tile96=16), dict(wide_db=1)):
        for c in pair:
            yield c, dict(DEFAULT_KNOBS, **over)
    for c in pair:
        yield dict(c, present=c["present"] | WARM), dict(DEFAULT_KNOBS)
    yield dict(pair[0], batch=0), dict(DEFAULT_KNOBS)      # empty output: nothing to launch


def attn_cases():
    sizes = (77, 200, 1000, 1024, 4096)
    for Nq, Nk, H, B, mask, ws, v in itertools.product(sizes, sizes, (5, 10, 20, 8), range(1, 9), (0, MASK), (0, XSPLIT_WS), (-1, 0, 1, 2, 6, 7, 8, 9)):
        yield dict(B=B, H=H, Nq=Nq, Nk=Nk, dt=F16, present=mask | ws, misaligned=0), dict(DEFAULT_KNOBS, attn_variant=v)
    for Nq, Nk, H, B in itertools.product(sizes, sizes, (5, 8), (1, 2)):
        c = dict(B=B, H=H, Nq=Nq, Nk=Nk, dt=F16, present=XSPLIT_WS, misaligned=0)
        yield dict(c, dt=F32), dict(DEFAULT_KNOBS)
        yield dict(c, misaligned=1), dict(DEFAULT_KNOBS)
        yield c, dict(DEFAULT_KNOBS, zero_page=0)
        yield c, dict(DEFAULT_KNOBS, attn_xsplit=0)


def is_default(knobs):
    return knobs == DEFAULT_KNOBS


def run(lib, which):
    """every case of `which` ("igemm" / "attn") through the library's debug entry -> (rows [n][fields + status] int32, error texts);
    status 0 = a choice, i > 0 = refused with texts[i - 1] (texts sorted, so the numbering does not depend on the order of the cases)"""
    entry, Case, Choice, fields, gen = ((lib.sdxl_debug_igemm_select, IgemmCase, IgemmChoice, IGEMM_CHOICE_FIELDS, igemm_cases) if which == "igemm" else
                                        (lib.sdxl_debug_attn_select, AttnCase, AttnChoice, ATTN_CHOICE_FIELDS, attn_cases))
    entry.restype = ctypes.c_int
    lib.sdxl_last_error.restype = ctypes.c_char_p
    rows, errors = [], []
    for case, knobs in gen():
        out = Choice()
        status = entry(ctypes.byref(Case(**case)), ctypes.byref(Knobs(**knobs)), ctypes.byref(out))
        if status != 0:
            msg = lib.sdxl_last_error().decode()
            if msg not in errors:
                errors.append(msg)
            rows.append([0] * len(fields) + [1 + errors.index(msg)])
        else:
            rows.append([getattr(out, f) for f in fields] + [0])
    rows, order = np.asarray(rows, dtype=np.int32), sorted(errors)
    rows[:, -1] = np.array([0] + [1 + order.index(e) for e in errors], dtype=np.int32)[rows[:, -1]]
    return rows, order
