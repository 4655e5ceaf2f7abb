"""The siblings' shared Python shell (bsarec_amd/_sibling.py) on the GPU, at the places where a generic shell can go
wrong while every per-model parity test still passes: operands that are misaligned or non-contiguous views (forward input and
incoming gradient), the workspace pool's take / give discipline, a second backward through one node, and FeaAttention (three
inputs, no weights) through the node the weight-bearing layers use.  Shapes: B = 3, d = 8; L = 9 for GRU, LRU and Mamba (one past
Mamba's 8-step checkpoint, so the backward forms states again across an edge), L = 12 for Caser and FeaAttention."""
import pytest
import torch

pytestmark = pytest.mark.gpu
B, D = 3, 8
FLAT = ["gru", "caser", "lru", "mamba"]
LAYERS = FLAT + ["fea"]


def _case(name, seed=0):
    """(layer on the GPU, its tensor inputs as fp32 values, the arguments behind them)."""
    from bsarec_amd.caser import CaserConv
    from bsarec_amd.fearec import FeaAttention
    from bsarec_amd.gru4rec import GruStack
    from bsarec_amd.lrurec import LruLayer
    from bsarec_amd.mamba4rec import MambaLayer
    torch.manual_seed(10 + seed)
    L = 12 if name in ("caser", "fea") else 9
    layer = {"gru": lambda: GruStack(D, 32, 1, D), "caser": lambda: CaserConv(12, D, 4, 1), "lru": lambda: LruLayer(D),
             "mamba": lambda: MambaLayer(D, d_state=4, d_conv=2, expand=2, dt_rank=4),
             "fea": lambda: FeaAttention(12, D, 0, 7, 2)}[name]().cuda()
    g = torch.Generator().manual_seed(seed)
    values = [torch.randn(B, L, D, generator=g).cuda() for _ in range(3 if name == "fea" else 1)]
    extra = ()
    if name in ("lru", "mamba"):
        ids = torch.randint(1, 50, (B, L), generator=g)
        ids[1, :4] = 0                                         # one left-padded row
        extra = (ids.cuda(),)
    return layer, values, extra


def _aligned(t):
    t = t.clone()
    assert t.is_contiguous() and t.data_ptr() % 16 == 0
    return t


def _misaligned(t):
    """The same values as a view 4 bytes off a 16-byte boundary."""
    buf = torch.empty(t.numel() + 4, dtype=t.dtype, device=t.device)
    view = buf[1:1 + t.numel()].view(t.shape)
    view.copy_(t)
    assert view.data_ptr() % 16 == 4
    return view


def _transposed(t):
    """The same values as a non-contiguous view: transposed, made contiguous, transposed back."""
    a, b = t.dim() - 2, t.dim() - 1
    view = t.transpose(a, b).contiguous().transpose(a, b)
    assert not view.is_contiguous() and torch.equal(view, t)
    return view


def _run(layer, values, extra, gout, form):
    """out, the inputs' gradients and the parameters' gradients of one forward + backward with every operand in ``form``."""
    for p in layer.flat_parameters():
        p.grad = None
    inputs = [form(v).detach().requires_grad_() for v in values]
    out = layer(*inputs, *extra)
    out.backward(form(gout))
    return [out.detach()] + [t.grad for t in inputs] + [p.grad for p in layer.flat_parameters()]


@pytest.mark.parametrize("form", [_misaligned, _transposed], ids=["misaligned", "non_contiguous"])
@pytest.mark.parametrize("name", LAYERS)
def test_operand_views_give_the_bits_of_the_aligned_call(name, form):
    layer, values, extra = _case(name)
    with torch.no_grad():
        shape = layer(*values, *extra).shape
    gout = torch.randn(shape, generator=torch.Generator().manual_seed(1)).cuda()
    want = _run(layer, values, extra, gout, _aligned)
    got = _run(layer, values, extra, gout, form)
    assert len(got) == len(want) == 1 + len(values) + len(layer._slices)
    for i, (a, b) in enumerate(zip(got, want)):
        assert a is not None and b is not None and bool(torch.isfinite(b).all()), i
        assert torch.equal(a, b), (name, i)
    assert any(bool((t != 0).any()) for t in want[1:])


def _free(layer):
    return [ws for pool in layer._pool.values() for ws in pool]


@pytest.mark.parametrize("name", LAYERS)
def test_pool_takes_and_gives_one_workspace_per_live_forward(name):
    layer, values, extra = _case(name)
    L = values[0].shape[1]
    inputs = [v.clone().requires_grad_() for v in values]
    assert _free(layer) == []
    out = layer(*inputs, *extra)
    assert _free(layer) == []                                # the backward's workspace is out of the pool
    out.sum().backward()
    assert len(_free(layer)) == 1
    (key,) = layer._pool
    assert key[:2] == (B, L) and len(layer._pool[key]) == 1
    first = _free(layer)[0].data_ptr()

    a, b = layer(*inputs, *extra), layer(*inputs, *extra)      # two forwards alive: the pooled workspace and a new one
    assert _free(layer) == []
    a.sum().backward()
    b.sum().backward()
    ptrs = sorted(ws.data_ptr() for ws in layer._pool[key])
    assert len(ptrs) == 2 and ptrs[0] != ptrs[1] and first in ptrs

    layer._pool.clear()
    with torch.no_grad():                                    # the evaluation-mode call takes one and gives it back
        layer(*values, *extra)
        assert len(_free(layer)) == 1
        kept = _free(layer)[0].data_ptr()
        layer(*values, *extra)
    assert [ws.data_ptr() for ws in _free(layer)] == [kept]


@pytest.mark.parametrize("name", FLAT)
def test_moves_keep_or_replace_the_flat_tensor(name):
    layer, values, extra = _case(name)
    x = values[0].clone().requires_grad_()
    layer(x, *extra).sum().backward()
    flat, values_before = layer._flat, [p.detach().clone() for p in layer.flat_parameters()]
    layer.cuda()                                             # already there: the address test holds, nothing is rebuilt
    assert layer._flat is flat
    layer.double().float()                                   # new storages: a new flat tensor, and the pool goes with the old one
    assert layer._flat is not flat and layer._pool == {}
    for p, v, (o, n, shp) in zip(layer.flat_parameters(), values_before, layer._slices.values()):
        assert p.data_ptr() == layer._flat.data_ptr() + 4 * o and torch.equal(p, v)
    layer(x, *extra).sum().backward()                        # and the layer runs on it
    assert len(_free(layer)) == 1


@pytest.mark.parametrize("name", LAYERS)
def test_second_backward_through_one_node_is_refused(name):
    layer, values, extra = _case(name)
    inputs = [v.clone().requires_grad_() for v in values]
    out = layer(*inputs, *extra)
    g = torch.ones_like(out)
    out.backward(g, retain_graph=True)
    with pytest.raises(RuntimeError, match="backward ran twice"):
        out.backward(g)
    assert len(_free(layer)) == 1                            # the workspace went back once


def test_fea_attention_runs_through_the_shared_node():
    from bsarec_amd import _sibling as S
    layer, values, extra = _case("fea")
    q, k, v = (t.clone().requires_grad_() for t in values)
    out = layer(q, k, v)
    assert type(out.grad_fn).__name__ == S._LayerFn.__name__ + "Backward"
    edges = lambda t: sum(fn is not None for fn, _ in t.grad_fn.next_functions)
    assert edges(out) == 3                                   # gradients go to q, k and v, and to nothing else
    gout = torch.randn(out.shape, generator=torch.Generator().manual_seed(2)).cuda()
    out.backward(gout)
    for t in (q, k, v):
        assert t.grad is not None and t.grad.shape == t.shape and bool(torch.isfinite(t.grad).all())
        assert bool((t.grad != 0).any())
    assert layer.flat_parameters() == [] and list(layer.parameters()) == []

    lru, lvalues, lextra = _case("lru")                      # a weight-bearing layer: the same node class
    y = lru(lvalues[0].clone().requires_grad_(), *lextra)
    assert type(y.grad_fn) is type(out.grad_fn)
    assert edges(y) == 1 + len(lru._slices) == 8             # x and the seven views
