"""Full ranking over a contiguous item range (bsarec_topk_full_range) and the fused evaluation of ShardedCatalogue, on the
host (no GPU): the symbol, the unchanged ABI version, the C99 header, the argument checks (which return < 0 before any HIP
call), the eval_full_rank validation, and the numpy statement of the partition rule the GPU tests rely on: the top-k of a
table cut into contiguous ranges is the merge, by (order key, global id), of the ranges' top-min(k, Vs) lists."""
import argparse
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import full_rank_ref as R
from conftest import ROOT


def test_library_exports_topk_full_range_at_abi_10():
    from bsarec_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.bsarec_abi_version() == 10
    assert hasattr(lib, "bsarec_topk_full_range") and "bsarec_topk_full_range" in _lib.EXPORTS
    header = open(os.path.join(ROOT, "include", "bsarec_hip.h")).read()
    assert "int bsarec_topk_full_range(const float *h, long ldh, const float *item_rows, int B, int Vs, long col_base, int d," in header


ORDER = ["h", "ldh", "item_rows", "B", "Vs", "col_base", "d", "users", "indptr", "indices", "k", "cand_cap", "workspace",
         "workspace_bytes", "out_idx", "out_val", "stream"]


def _valid_call():
    buf = (C.c_byte * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16       # a 16-byte aligned host address (never dereferenced)
    return buf, dict(h=p, ldh=64, item_rows=p, B=4, Vs=100, col_base=300, d=64, users=p, indptr=None, indices=None, k=20,
                     cand_cap=0, workspace=p, workspace_bytes=1 << 40, out_idx=p, out_val=None, stream=None)


# every case bsarec_topk_full refuses (tests/test_full_rank_cpu.py), then the range's own
@pytest.mark.parametrize("change", [dict(k=0), dict(k=1025), dict(Vs=19), dict(B=0), dict(d=2), dict(d=260), dict(d=66),
                                    dict(ldh=32), dict(h=None), dict(item_rows=None), dict(workspace=None), dict(out_idx=None),
                                    dict(indptr="p"), dict(indptr="p", users=None), dict(item_rows="p+4"), dict(h="p+4"),
                                    dict(workspace="p+4"), dict(cand_cap=19), dict(cand_cap=-1), dict(workspace_bytes=1000),
                                    dict(col_base=-1), dict(col_base=2**31 - 100), dict(col_base=2**31 - 1),
                                    dict(col_base=2**40), dict(Vs=2**31 - 1, col_base=1)])
def test_invalid_arguments_return_negative_without_a_gpu(change):
    from bsarec_amd import _lib
    lib = _lib.load()
    buf, kw = _valid_call()
    p = kw["h"]
    for k, v in change.items():
        kw[k] = {"p": p, "p+4": p + 4}.get(v, v) if isinstance(v, str) else v
    assert lib.bsarec_topk_full_range(*[kw[k] for k in ORDER]) < 0


def test_short_workspace_is_refused():
    from bsarec_amd import _lib
    lib = _lib.load()
    buf, kw = _valid_call()
    kw["workspace_bytes"] = lib.bsarec_topk_full_workspace_bytes(4, 100, 64, 20, 0) - 1
    assert lib.bsarec_topk_full_range(*[kw[k] for k in ORDER]) < 0


def test_header_declares_topk_full_range_for_c99(tmp_path):
    """A C99 program that includes the header compiles, links against the library and gets < 0 from invalid calls."""
    lib_dir = os.path.join(ROOT, "bsarec_amd")
    if not os.path.exists(os.path.join(lib_dir, "libbsarec_hip.so")) or not shutil.which("gcc"):
        pytest.skip("library or gcc missing")
    src = r"""
#include "bsarec_hip.h"
#include <stdio.h>
int main(void) {
    static float h[64 * 4], e[64 * 100];
    static int64_t idx[4 * 20];
    long ws = bsarec_topk_full_workspace_bytes(4, 100, 64, 20, 0);
    int bad_k = bsarec_topk_full_range(h, 64, e, 4, 100, 300, 64, NULL, NULL, NULL, BSAREC_TOPK_MAX + 1, 0, h, ws, idx, NULL, NULL);
    int bad_lo = bsarec_topk_full_range(h, 64, e, 4, 100, -1, 64, NULL, NULL, NULL, 20, 0, h, ws, idx, NULL, NULL);
    int bad_hi = bsarec_topk_full_range(h, 64, e, 4, 100, 2147483647L - 99, 64, NULL, NULL, NULL, 20, 0, h, ws, idx, NULL, NULL);
    int bad_ws = bsarec_topk_full_range(h, 64, e, 4, 100, 300, 64, NULL, NULL, NULL, 20, 0, h, ws - 1, idx, NULL, NULL);
    printf("%d %ld %d %d %d %d\n", bsarec_abi_version(), ws, bad_k, bad_lo, bad_hi, bad_ws);
    return (bsarec_abi_version() == 10 && ws > 0 && bad_k < 0 && bad_lo < 0 && bad_hi < 0 && bad_ws < 0) ? 0 : 1;
}
"""
    f = tmp_path / "host.c"
    f.write_text(src)
    exe = tmp_path / "host"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe),
                    "-L", lib_dir, "-lbsarec_hip", f"-Wl,-rpath,{lib_dir}"], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def _ns(**kw):
    a = argparse.Namespace(item_size=301, hidden_size=64, max_seq_length=50, batch_size=32, hidden_dropout_prob=0.0,
                           attention_probs_dropout_prob=0.0, num_hidden_layers=2, num_attention_heads=2,
                           hidden_act="gelu", initializer_range=0.02, c=3, alpha=0.9, seed=42, lr=1e-3,
                           adam_beta1=0.9, adam_beta2=0.999, weight_decay=0.0, no_cuda=False, log_freq=1)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


def test_eval_full_rank_is_validated_before_the_device_check():
    from bsarec_amd.catalogue import ShardedCatalogue, eval_full_rank_of
    with pytest.raises(ValueError, match="eval_full_rank"):
        ShardedCatalogue(_ns(eval_full_rank="sparse"), 32, None, "cpu")
    with pytest.raises(ValueError, match="eval_full_rank"):
        ShardedCatalogue(_ns(eval_full_rank="sparse", train_negatives=64), 32, None, "cpu")
    for ok in (dict(), dict(eval_full_rank="dense"), dict(eval_full_rank="fused")):
        with pytest.raises(ValueError, match="runs on the GPU only"):       # a valid flag reaches the device check
            ShardedCatalogue(_ns(**ok), 32, None, "cpu")
    # the validator topk(..., full_rank=) and full_sort_scores(..., full_rank=) go through
    assert eval_full_rank_of(_ns()) == "dense"
    assert eval_full_rank_of(_ns(eval_full_rank="fused")) == "fused"
    assert eval_full_rank_of(_ns(eval_full_rank="fused"), "dense") == "dense"
    assert eval_full_rank_of(_ns(), "fused") == "fused"
    for bad in ("sparse", "", "Fused", 1):
        with pytest.raises(ValueError, match="eval_full_rank"):
            eval_full_rank_of(_ns(), bad)
    with pytest.raises(ValueError, match="eval_full_rank"):
        eval_full_rank_of(_ns(eval_full_rank="sparse"))
    assert eval_full_rank_of(_ns(eval_full_rank="sparse"), "fused") == "fused"


def merge_parts(scores, seen_global, k, bounds):
    """Per contiguous part [lo, hi): the top-min(k, hi - lo) of the slice with GLOBAL seen ids mapped by the range rule (an id
    applies iff lo <= id < hi), output ids shifted by lo; then the merge by (order key, global id)."""
    B = scores.shape[0]
    ids_parts, val_parts = [], []
    for lo, hi in bounds:
        kk = min(k, hi - lo)
        if kk == 0:
            continue
        local = [[g - lo for g in row if lo <= g < hi] for row in seen_global]
        i, v = R.topk(scores[:, lo:hi], local, kk)
        ids_parts.append(i + lo)
        val_parts.append(v)
    ids, vals = np.concatenate(ids_parts, 1), np.concatenate(val_parts, 1)
    out_i, out_v = np.empty((B, k), np.int64), np.empty((B, k), np.float32)
    for b in range(B):
        # NaN first (order_keys gives NaN and +inf the same key), then the key ascending, then the smaller global id
        order = np.lexsort((ids[b], R.order_keys(vals[b]), ~np.isnan(vals[b])))
        out_i[b], out_v[b] = ids[b][order[:k]], vals[b][order[:k]]
    return out_i, out_v


def contiguous_bounds(V, W):
    rows_per = (V + W - 1) // W
    return [(min(V, r * rows_per), min(V, (r + 1) * rows_per)) for r in range(W)]


@pytest.mark.parametrize("kind", ["float", "ties", "special"])
@pytest.mark.parametrize("V,k,bounds", [
    (40, 20, contiguous_bounds(40, 2)), (40, 20, contiguous_bounds(40, 3)), (40, 20, contiguous_bounds(40, 8)),
    (302, 20, contiguous_bounds(302, 3)), (1000, 100, contiguous_bounds(1000, 8)), (37, 20, contiguous_bounds(37, 8)),
    (5, 5, contiguous_bounds(5, 8)), (500, 20, [(0, 7), (7, 320), (320, 333), (333, 500)]), (500, 1, [(0, 499), (499, 500)]),
])
def test_partition_merge_equals_the_whole_table(kind, V, k, bounds):
    rng = np.random.default_rng(V * 31 + k + len(bounds))
    B = 9
    if kind == "float":
        s = rng.standard_normal((B, V)).astype(np.float32)
    elif kind == "ties":
        s = rng.integers(-2, 3, size=(B, V)).astype(np.float32)          # five values: heavy ties across the parts
        s[1] = 0.0
        s[2] = -1.0                                                      # all negative: the seen zeros win
    else:
        s = rng.integers(-1, 2, size=(B, V)).astype(np.float32)
        s[s == 0] = np.where(rng.random((s == 0).sum()) < 0.5, -0.0, 0.0).astype(np.float32)
        s[rng.random((B, V)) < 0.1] = np.nan
        s[rng.random((B, V)) < 0.05] = np.inf
        s[rng.random((B, V)) < 0.05] = -np.inf
        s[3] = np.nan
    seen = []
    for b in range(B):
        row = rng.integers(0, V, size=int(rng.integers(0, 2 * V))).tolist()      # duplicates included
        row += [-1] * 3 + [V, V + 7, -5]                                          # pads and ids outside the catalogue
        seen.append(row)
    assert bounds[0][0] == 0 and bounds[-1][1] == V and all(p[1] == q[0] for p, q in zip(bounds, bounds[1:]))
    want_i, want_v = R.topk(s, seen, k)
    got_i, got_v = merge_parts(s, seen, k, bounds)
    np.testing.assert_array_equal(got_i, want_i)
    np.testing.assert_array_equal(got_v.view(np.uint32), want_v.view(np.uint32))
