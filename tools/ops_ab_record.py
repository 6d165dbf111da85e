"""Bit-level A/B of two builds of the library over the single-op entries.  pytest plugin: wraps the package's single-op functions and stores what every call returns (or the error text it
raises) per test, so two libraries can be compared bit for bit over exactly the calls the op tests make.  One process per library (SDXL_LIB_PATH names the other build):

    RECORD_OPS_DIR=/tmp/a SDXL_LIB_PATH=<other .so> PYTHONPATH=tools python -m pytest -m gpu -p ops_ab_record \
        tests/test_gpu_ops.py tests/test_gpu_f16_kernels.py tests/test_gpu_forms.py tools/ops_ab_cases.py
    RECORD_OPS_DIR=/tmp/b PYTHONPATH=tools python -m pytest -m gpu -p ops_ab_record <the same files>
    python tools/ops_ab_compare.py /tmp/a /tmp/b "other vs this"

The recordings are large (about 6 GB per run for the three op test files): keep them out of the repository."""
import hashlib
import os

import numpy as np

OPS = ["qkv_attention", "attn_decoder_mask", "group_norm", "layer_norm", "conv2d", "linear", "layer_norm_linear",
       "ln_query_cross_attention", "transformer_projection", "conv2d_group_norm"]
if os.environ.get("RECORD_OPS"):      # a comma-separated subset, e.g. the attention entries only
    OPS = [n for n in OPS if n in os.environ["RECORD_OPS"].split(",")]
OUT = os.environ["RECORD_OPS_DIR"]
_calls = []
_n = [0]


def _flat(name, v, dst):
    import torch
    if isinstance(v, torch.Tensor):
        dst[name] = v.detach().cpu().numpy()
    elif isinstance(v, (tuple, list)):
        for i, e in enumerate(v):
            _flat(f"{name}_{i}", e, dst)
    elif v is None:
        dst[name] = np.zeros(0)
    else:
        dst[name] = np.asarray(v)


def _wrap(name, fn):
    def w(*a, **k):
        key = f"c{len(_calls):04d}_{name}"
        d = {}
        try:
            r = fn(*a, **k)
        except Exception as e:
            d[key + "_error"] = np.frombuffer(str(e).encode(), dtype=np.uint8)
            _calls.append(d)
            raise
        _flat(key, r, d)
        _calls.append(d)
        return r
    return w


def pytest_sessionstart(session):
    import __graft_entry__ as ge
    pkg = ge.load_package()
    os.makedirs(OUT, exist_ok=True)
    for n in OPS:
        setattr(pkg, n, _wrap(n, getattr(pkg, n)))
    print("ops_ab_record: library", pkg.LIB_PATH)


def pytest_runtest_teardown(item):
    if _calls:
        d = {}
        for c in _calls:
            d.update(c)
        h = hashlib.sha1(item.nodeid.encode()).hexdigest()[:10]
        np.savez(os.path.join(OUT, f"{_n[0]:05d}_{h}.npz"), nodeid=np.frombuffer(item.nodeid.encode(), dtype=np.uint8), **d)
        _calls.clear()
    _n[0] += 1
