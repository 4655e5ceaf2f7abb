"""The host side of a fused pairwise step (one C call per optimisation step), once for GRU4RecModel and CaserModel: the buffers
beside the parameters, the per-shape slots, the Adam structs and the eager / warm-up / capture / replay sequence.  A model brings
its arrays as ``(tag, tensor)`` pairs -- the item table is tagged "E" -- its config with the workspace size, and its two C calls."""
import torch

from . import _lib as L


def buffers(f, arrays, seed: int):
    """The dict a model keeps in ``_fused``: ``f`` itself while the arrays' storages are the ones it was built on, else a new one
    with the device step state int64[8] (``state``: [0] = ``seed``, the step counter and Adam's t at 0) and per array ``tag`` the
    tensor under ``tag``, its gradient under "d" + tag and zeroed Adam moments under "m" + tag and "v" + tag; ``slots`` is empty
    and ``adam`` unset."""
    dev = arrays[0][1].device
    key = tuple(t.data_ptr() for _, t in arrays) + (dev,)
    if f is not None and f["key"] == key:
        return f
    state = torch.zeros(8, dtype=torch.int64, device=dev)
    state[0] = seed
    f = dict(key=key, state=state, tags=tuple(tag for tag, _ in arrays), adam=None, slots={})
    for tag, t in arrays:
        f[tag], f["d" + tag], f["m" + tag], f["v" + tag] = t, torch.empty_like(t), torch.zeros_like(t), torch.zeros_like(t)
    return f


def slot(f, key, cfg, nbytes: int, ids_shape, extra=()):
    """What one batch shape owns, kept under ``f["slots"][key]``: the workspace, static id buffers (``ids`` of ``ids_shape`` =
    (B, L); ``ans``, ``neg`` and every name of ``extra`` [B]), the loss scalar and the captured graph (None until captured)."""
    dev = f["state"].device
    ids = lambda *shape: torch.zeros(shape, dtype=torch.int64, device=dev)
    B = ids_shape[0]
    s = dict(cfg=cfg, nbytes=nbytes, ws=torch.empty(nbytes, dtype=torch.uint8, device=dev), ids=ids(*ids_shape), ans=ids(B),
             neg=ids(B), loss=torch.zeros((), dtype=torch.float32, device=dev), graph=None)
    for name in extra:
        s[name] = ids(B)
    f["slots"][key] = s
    return s


def stream(f) -> int:
    return torch.cuda.current_stream(f["state"].device).cuda_stream


def adam_structs(f, args):
    """One bsarec_adam_t per array, in the arrays' order, with ``args.lr`` / ``adam_beta1`` / ``adam_beta2`` / ``weight_decay``."""
    if f["adam"] is None:
        hyper = (float(getattr(args, "lr", 1e-3)), float(getattr(args, "adam_beta1", 0.9)), float(getattr(args, "adam_beta2", 0.999)),
                 1e-8, float(getattr(args, "weight_decay", 0.0)), 1.0, None, 0)
        f["adam"] = tuple(L.Adam(f[t].data_ptr(), f["d" + t].data_ptr(), f["m" + t].data_ptr(), f["v" + t].data_ptr(), f[t].numel(),
                                 *hyper) for t in f["tags"])
    return f["adam"]


def train_step(f, s, args, graph: bool, loss_grad, step):
    """One optimisation step on the filled slot ``s`` through ``step(f, s)``: eagerly, or captured once per slot and replayed.
    Returns the slot's loss scalar (no host sync)."""
    if not graph:
        step(f, s)
        return s["loss"]
    if s["graph"] is None:
        adam_structs(f, args)
        loss_grad(f, s, False)                            # every kernel of the chain has run once before the capture; no
        g = torch.cuda.CUDAGraph()                        # counter moves and nothing is updated (train = 0)
        with torch.cuda.graph(g):
            step(f, s)
        s["graph"] = g
    s["graph"].replay()
    return s["loss"]
