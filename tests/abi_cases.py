"""The host-side checks that every one-call training step's *_cpu.py file makes of its entry points, once: the list of invalid
argument cases, the engine that turns a case into an argument list (``build``) and the call itself (``call``), the exported-symbols
check, the C99 compile-and-link runner and the command-line-flag check.  A file describes its entry points with ``spec`` and keeps
its own GOOD, BAD_CFG, signatures, pointer classes and config constructor.

The entry points are handed HOST addresses: every case must make the call invalid, so that it returns < 0 before any HIP call.
``build`` exists apart from ``call`` so that the arguments of every case can be looked at without calling the library."""
import ctypes as C
import os
import shutil
import subprocess
import types

import pytest

from conftest import ROOT

ADAM_PTRS = ["params", "grads", "exp_avg", "exp_avg_sq"]
ADAM_OPTIONS = (("shadow_bf16", "p"), ("grads2", "p"), ("grads2_n", 4), ("n_grad_srcs", 1), ("wimage_plan", "p"))    # all refused
ONE_RATE = [{"adam_weights.lr": 2e-3}, {"adam_weights.beta1": 0.8}, {"adam_items.beta2": 0.99}]    # one lr, beta1, beta2 per step
_BUF = (C.c_byte * 4096)()           # host memory whose aligned address every case passes as a pointer: never dereferenced


def spec(good, cfg, entry, ptrs16, ptrs8, need, adam_n, sizes=None):
    """good: the valid config's fields; cfg(**changes) -> the config struct; entry: {entry name: argument names}; ptrs16 /
    ptrs8: the pointer arguments as ``step_cases`` takes them -- with loss_out they are the ONLY arguments that get the host
    address; need(lib) -> workspace bytes of the valid config; adam_n(lib) -> {Adam argument: its n}; sizes(lib) -> further
    named workspace sizes beside "short"."""
    pointers = sorted({p for ps in ptrs16.values() for p in ps} | set(ptrs8) | {"loss_out"})
    return types.SimpleNamespace(good=good, cfg=cfg, entry=entry, pointers=pointers, need=need, adam_n=adam_n, sizes=sizes)


def step_cases(entry, bad_cfg, ptrs16, ptrs8, adams=("adam_items", "adam_weights"), adams_in_full=None, sizes=(0, "short"),
               hyper=ONE_RATE):
    """The (entry name, change) list of a loss_grad / train_step pair.  ``adams_in_full``: the Adam structs whose pointers and
    refused options are walked through (default: all of ``adams``); ``hyper``: the changes of one struct's lr / beta1 / beta2."""
    T = next(n for n in entry if n.endswith("_train_step"))
    full = adams if adams_in_full is None else adams_in_full
    cases = [(n, c) for n in entry for c in bad_cfg] + [(n, dict(cfg=None)) for n in entry]
    cases += [(n, {p: v}) for n in entry for p in ptrs16[n] + ptrs8 for v in (None, "p+4")]
    cases += [(n, dict(loss_out=v)) for n in entry for v in (None, "p+2")]
    cases += [(n, dict(workspace_bytes=v)) for n in entry for v in sizes]
    cases += [(T, {a: None}) for a in adams]
    cases += [(T, {f"{a}.{p}": v}) for a in full for p in ADAM_PTRS for v in (None, "p+4")]
    cases += [(T, {f"{a}.n": v}) for a in adams for v in ("n+4", "n-4", 0)]
    cases += [(T, {f"{a}.{k}": v}) for a in full for k, v in ADAM_OPTIONS]
    return cases + [(T, c) for c in hyper]


def ids(cases, prefix):
    """The parametrised ids: the entry name without ``prefix`` (bsarec_<model>_), then every change."""
    return [f"{n[len(prefix):]}-" + "-".join(f"{k}={v}" for k, v in c.items()) for n, c in cases]


def build(s, name, change):
    """-> (entry name, argument list) of one case: every pointer the 16-byte aligned host address p (never dereferenced), the
    valid config and workspace size, valid Adam structs -- and then the change.  An argument name that is neither one of the
    spec's pointers nor cfg, train, workspace_bytes, stream or an Adam is a KeyError, not a host address."""
    from bsarec_amd import _lib
    lib = _lib.load()
    p = C.addressof(_BUF) + (-C.addressof(_BUF)) % 16
    need, n = s.need(lib), s.adam_n(lib)
    adam = {a: _lib.Adam(p, p, p, p, n[a], 1e-3, 0.9, 0.999, 1e-8, 0.0, 1.0, None, 0) for a in n}
    kw = {k: p for k in s.pointers}
    kw.update(cfg=s.cfg(), train=1, workspace_bytes=need, stream=None, **adam)
    named = {"p+4": p + 4, "p+2": p + 2, "short": need - 1}
    if s.sizes is not None:
        named.update(s.sizes(lib))
    for k, v in change.items():
        if k in s.good:
            kw["cfg"] = s.cfg(**change)
        elif "." in k:
            a, field = k.split(".")
            v = {"p": p, "p+4": p + 4, "n+4": n[a] + 4, "n-4": n[a] - 4}.get(v, v) if isinstance(v, str) else v
            if field == "n_grad_srcs":
                adam[a].grad_srcs[0] = p
            setattr(adam[a], field, v)
        else:
            kw[k] = named.get(v, v) if isinstance(v, str) else v
    return name, [kw[k] for k in s.entry[name]]


def call(s, name, change):
    from bsarec_amd import _lib
    name, args = build(s, name, change)
    return getattr(_lib.load(), name)(*args)


def check_symbols(names, nargs, struct, fields, size):
    """Every name exported and bound as _lib.EXPORTS says; ``nargs``: {entry name: argument count}; the config struct's fields
    and size; the ABI version, which an additive change leaves."""
    from bsarec_amd import _lib
    lib = _lib.load()
    for name in names:
        assert name in _lib.EXPORTS
        assert getattr(lib, name).argtypes == _lib.EXPORTS[name][1]
        assert getattr(lib, name).restype == _lib.EXPORTS[name][0]
    for name, n in nargs.items():
        assert name in names and len(_lib.EXPORTS[name][1]) == n, name
    assert [f for f, _ in struct._fields_] == fields
    assert C.sizeof(struct) == size
    assert lib.bsarec_abi_version() == 10 and _lib.ABI_VERSION == 10


def run_c99(tmp_path, src):
    """Compile ``src`` as C99 with -Wall -Werror against the header, link it with the library, run it: it must return 0.
    -> the integers it printed."""
    lib_dir = os.path.join(ROOT, "bsarec_amd")
    if not os.path.exists(os.path.join(lib_dir, "libbsarec_hip.so")) or not shutil.which("gcc"):
        pytest.skip("library or gcc missing")
    f = tmp_path / "host.c"
    f.write_text(src)
    exe = tmp_path / "host"
    subprocess.run(["gcc", "-std=c99", "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(f), "-o", str(exe),
                    "-L", lib_dir, "-lbsarec_hip", f"-Wl,-rpath,{lib_dir}"], check=True, capture_output=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return [int(v) for v in r.stdout.split()]


def check_flag(flag, model_type):
    """--<flag> {torch, fused}: absent unless given (the logged arguments stay as they were), no third value."""
    from bsarec_amd.main import parse_args
    assert not hasattr(parse_args([]), flag)
    assert getattr(parse_args(["--model_type", model_type, "--" + flag, "fused"]), flag) == "fused"
    assert getattr(parse_args(["--" + flag, "torch"]), flag) == "torch"
    with pytest.raises(SystemExit):
        parse_args(["--" + flag, "graph"])
