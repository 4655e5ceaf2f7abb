"""Full-catalogue top-k without the score matrix, on the host (no GPU): the C entry points' symbols, ABI version, workspace
query and argument checks (which return < 0 before any HIP call), the C99 header, the --eval_full_rank flag and the numpy
restatement of the ranking order."""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

torch = pytest.importorskip("torch")

import full_rank_ref as R
from conftest import ROOT
from oracle import bsarec_oracle as O


def test_library_exports_topk_full_at_abi_10():
    from bsarec_amd import _lib
    lib = _lib.load()
    assert _lib.ABI_VERSION == 10 and lib.bsarec_abi_version() == 10
    assert hasattr(lib, "bsarec_topk_full") and hasattr(lib, "bsarec_topk_full_workspace_bytes")
    header = open(os.path.join(ROOT, "include", "bsarec_hip.h")).read()
    assert "long bsarec_topk_full_workspace_bytes(int B, int V, int d, int k, int cand_cap);" in header


def test_workspace_query_limits_and_sizes():
    from bsarec_amd import _lib
    q = _lib.load().bsarec_topk_full_workspace_bytes
    assert q(256, 1_000_003, 64, 20, 0) == q(256, 1_000_003, 64, 20, 0) > 0
    assert q(256, 1_000_003, 64, 20, 0) <= 64 << 20            # the score matrix: 1 GB
    assert q(256, 1_000_003, 64, 1024, 0) <= 256 << 20
    sizes = [q(256, 100_003, 64, 20, c) for c in (20, 37, 1000, 5000, 100_000)]
    assert all(a < b for a, b in zip(sizes, sizes[1:]))
    for args in [(1, 1, 4, 1, 0), (257, 4097, 256, 1024, 0), (3, 1000, 16, 100, 100), (1, 2**31 - 1, 64, 20, 0)]:
        assert q(*args) > 0, args
    for args in [(0, 100, 64, 20, 0), (1, 100, 64, 0, 0), (1, 100, 64, 1025, 0), (1, 10, 64, 20, 0), (1, 100, 66, 20, 0),
                 (1, 100, 2, 1, 0), (1, 100, 260, 20, 0), (1, 100, 64, 20, 19), (1, 100, 64, 20, -1)]:
        assert q(*args) < 0, args


ORDER = ["h", "ldh", "item_emb", "B", "V", "d", "users", "indptr", "indices", "k", "cand_cap", "workspace", "workspace_bytes",
         "out_idx", "out_val", "stream"]


def _valid_call():
    buf = (C.c_byte * 4096)()
    p = C.addressof(buf) + (-C.addressof(buf)) % 16       # a 16-byte aligned host address (never dereferenced)
    return buf, dict(h=p, ldh=64, item_emb=p, B=4, V=100, d=64, users=p, indptr=None, indices=None, k=20, cand_cap=0,
                     workspace=p, workspace_bytes=1 << 40, out_idx=p, out_val=None, stream=None)


@pytest.mark.parametrize("change", [dict(k=0), dict(k=1025), dict(V=19), dict(B=0), dict(d=2), dict(d=260), dict(d=66),
                                    dict(ldh=32), dict(h=None), dict(item_emb=None), dict(workspace=None), dict(out_idx=None),
                                    dict(indptr="p"), dict(indptr="p", users=None), dict(item_emb="p+4"), dict(h="p+4"),
                                    dict(workspace="p+4"), dict(cand_cap=19), dict(cand_cap=-1), dict(workspace_bytes=1000)])
def test_invalid_arguments_return_negative_without_a_gpu(change):
    from bsarec_amd import _lib
    lib = _lib.load()
    buf, kw = _valid_call()
    p = kw["h"]
    for k, v in change.items():
        kw[k] = {"p": p, "p+4": p + 4}.get(v, v) if isinstance(v, str) else v
    assert lib.bsarec_topk_full(*[kw[k] for k in ORDER]) < 0


def test_short_workspace_is_refused():
    from bsarec_amd import _lib
    lib = _lib.load()
    buf, kw = _valid_call()
    kw["workspace_bytes"] = lib.bsarec_topk_full_workspace_bytes(4, 100, 64, 20, 0) - 1
    assert lib.bsarec_topk_full(*[kw[k] for k in ORDER]) < 0


def test_header_declares_topk_full_for_c99(tmp_path):
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
    int bad_k = bsarec_topk_full(h, 64, e, 4, 100, 64, NULL, NULL, NULL, BSAREC_TOPK_MAX + 1, 0, h, ws, idx, NULL, NULL);
    int bad_d = bsarec_topk_full(h, 64, e, 4, 100, 66, NULL, NULL, NULL, 20, 0, h, ws, idx, NULL, NULL);
    printf("%d %ld %d %d\n", bsarec_abi_version(), ws, bad_k, bad_d);
    return (ws > 0 && bad_k < 0 && bad_d < 0) ? 0 : 1;
}
"""
    f = tmp_path / "host.c"
    f.write_text(src)
    exe = tmp_path / "host"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe),
                    "-L", lib_dir, "-lbsarec_hip", f"-Wl,-rpath,{lib_dir}"], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr


def test_eval_full_rank_flag():
    from bsarec_amd.main import parse_args
    a = parse_args([])
    assert not hasattr(a, "eval_full_rank") and "eval_full_rank" not in str(a)
    assert parse_args(["--eval_full_rank", "fused"]).eval_full_rank == "fused"
    assert parse_args(["--eval_full_rank", "dense"]).eval_full_rank == "dense"
    assert parse_args(["--eval_full_rank", "fused", "--eval_negatives", "0"]).eval_full_rank == "fused"
    with pytest.raises(SystemExit):
        parse_args(["--eval_full_rank", "fused", "--eval_negatives", "100"])
    with pytest.raises(SystemExit):
        parse_args(["--eval_full_rank", "sparse"])


def test_restatement_matches_the_oracle_on_tie_free_rows():
    rng = np.random.default_rng(3)
    s = rng.standard_normal((6, 500)).astype(np.float32)
    seen = [rng.choice(500, size=n, replace=False).tolist() for n in (0, 1, 5, 30, 100, 499)]
    for b in range(6):          # tie-free: each row keeps at most one zero
        s[b, 0] = 1e-3 + b
    ids, vals = R.topk(s, seen, 20)
    want = O.topk_after_seen(s, seen, 20)
    for b in range(6):
        if len(seen[b]) <= 1:
            np.testing.assert_array_equal(ids[b], want[b])
        m = R.masked(s[b:b + 1], seen[b:b + 1])[0]
        np.testing.assert_array_equal(vals[b], m[ids[b]])


def test_restatement_order_rules():
    s = np.array([[0.0, -0.0, np.nan, 1.0, np.inf, np.nan, -1.0, 0.0]], np.float32)
    ids, vals = R.topk(s, [[3]], 8)
    # NaNs first (smaller column first), +inf, then the zeros (-0 = +0, seen 3 is 0) by column, then -1
    assert ids[0].tolist() == [2, 5, 4, 0, 1, 3, 7, 6]
    assert vals[0, 5] == 0.0
