"""Shared by the tests of MetaDOAR training (cygym_meta_select, cygym_amd/meta_rollout.py; CPU and GPU): the float64 restatement of the
observer's selection (policies.MetaNet.observe) with the bound of an fp32 evaluation's error on its scores and on the pooled embedding,
derived in float64 from sums of absolute terms by the method of tests/meta_util.py."""
import os

import numpy as np
import torch

from cygym_amd import spec as S
from cygym_amd.policies import MetaNet
from meta_util import _f64, _g, _layer, U

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "meta_train")
FIXTURES = ("def12", "att20")
NAMES = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias")
_FIX = {}


def load_fixture(name):
    """(arrays of tests/golden/meta_train/<name>.npz, the initial strategy mapping as tensors, a MetaNet holding it); loaded once, shared
    and left unchanged.  dims = (state_dim, M, k, role code, traces, decisions, batch_size).  tools/make_meta_train_golden.py records it."""
    if name not in _FIX:
        z = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
        assert all(v.dtype.kind in "fiub" for v in z.values()), "a fixture holds arrays of numbers only"
        mapping = {key: {k[len("sd." + key) + 1:]: torch.from_numpy(v) for k, v in z.items() if k.startswith("sd." + key + ".")}
                   for key in ("state_proj", "node_proj", "struct_feats")}
        _FIX[name] = (z, mapping, MetaNet.from_mapping({"meta": mapping}).eval())
    return _FIX[name]


@torch.no_grad()
def observe64(net, state, flags, adj, role, k, feat=None, selected=None):
    """MetaNet.observe in float64 and the bounds of an fp32 evaluation's error:
      score [n, M]   as meta_util.restate derives it: the polynomial sum_p proj_p (b2_p + sum_e W2[p][e] relu(x_ie)) evaluated in any
                     order differs from its exact value by at most g(ED + P + 2) times the polynomial of absolute values, plus what the
                     errors of proj and of x contribute through it
      ebar [n, P]    E_ip = b2_p + sum_e W2[p][e] relu(x_ie): g(ED) (|b2_p| + sum_e |W2| relu(x)) + sum_e |W2| err(x_ie) per device
                     (relu is 1-Lipschitz); the sum over n_sel <= 32 devices and the product with fl(1 / n_sel) -- an INPUT of the
                     stated formula -- add g(n_sel + 1) times the sum of absolute values; all of it times 1 / n_sel
    x_ie = base (id_dim terms, an fp32 table: g(id_dim) |.|) + three adds (g(3) |.|); degn is an input (the exact fp32 quotient, or the
    snapshot's).  Returns (observe's dict, {"score": bound, "ebar": bound})."""
    out = net.observe(state.cpu(), flags, adj, role, k, feat=feat, dtype=torch.float64, selected=selected)
    s = _f64(state)
    sp, ID = net.state_proj, net.id_dim
    h, e_h = _layer(_f64(sp.fc1.weight), _f64(sp.fc1.bias), s)
    proj, e_proj = _layer(_f64(sp.fc2.weight), _f64(sp.fc2.bias), torch.relu(h), e_h)
    w0, b0 = _f64(net.node_proj[0].weight), _f64(net.node_proj[0].bias)
    base, e_base = _layer(w0[:, :ID], b0, _f64(net.struct_feats.id_emb.weight))                  # [M, ED]
    degn, known, owned = (t.double() for t in out["feat"])
    x = base[None] + degn[:, :, None] * w0[:, ID] + known[:, :, None] * w0[:, ID + 1] + owned[:, :, None] * w0[:, ID + 2]
    x_abs = base.abs()[None] + degn[:, :, None] * w0[:, ID].abs() + known[:, :, None] * w0[:, ID + 1].abs() + owned[:, :, None] * w0[:, ID + 2].abs()
    e_x = e_base[None] + _g(3) * x_abs
    w2, b2 = _f64(net.node_proj[2].weight), _f64(net.node_proj[2].bias)
    emb_abs = torch.relu(x) @ w2.abs().t() + b2.abs()                                             # [n, M, P]
    e_emb_in = e_x @ w2.abs().t()
    s_abs = (emb_abs * proj.abs()[:, None, :]).sum(dim=2)
    b_score = (_g(net.embed_dim + net.proj_dim + 2) * s_abs + (e_emb_in * proj.abs()[:, None, :]).sum(dim=2)
               + ((emb_abs + e_emb_in) * e_proj[:, None, :]).sum(dim=2))
    sel = out["sel"]
    keep = (sel >= 0).double()
    rows = torch.arange(sel.shape[0])
    e_emb = _g(net.embed_dim) * emb_abs + e_emb_in
    sum_err, sum_abs = torch.zeros_like(proj), torch.zeros_like(proj)
    for j in range(sel.shape[1]):
        d = sel[:, j].clamp(min=0)
        sum_err = sum_err + e_emb[rows, d] * keep[:, j:j + 1]
        sum_abs = sum_abs + emb_abs[rows, d] * keep[:, j:j + 1]
    n_sel = out["n_sel"].double()
    inv = torch.where(n_sel > 0, 1.0 / n_sel.clamp(min=1), torch.zeros_like(n_sel))[:, None]
    b_ebar = inv * (sum_err + _g(n_sel[:, None] + 1) * sum_abs) + U * out["ebar"].abs()            # (+ the rounding of the stored value)
    return out, {"score": b_score, "ebar": b_ebar}


def trace64(net, states, flags, adj, role, k, selected=None):
    """One trace (decisions as rows: states [D, W], flags [D, M]) as the reference's observer sees it: the structural features of the
    FIRST decision for every decision, visibility of each decision's own flags.  Returns (the frozen restatement, its bounds, the live
    restatement of the same decisions)."""
    first, _ = observe64(net, states[:1], flags[:1], adj, role, k)
    D = int(states.shape[0])
    feat = tuple(t.expand(D, -1) for t in first["feat"])
    frozen, bnd = observe64(net, states, flags, None, role, k, feat=feat, selected=selected)
    live, _ = observe64(net, states, flags, adj, role, k)
    return frozen, bnd, live


def bits(a):
    """fp32 values as their bit patterns (bit-equality, NaN included)."""
    return np.ascontiguousarray(np.asarray(a, np.float32)).view(np.int32)


def other_flags(flags, role, seed):
    """Flag planes of the same shape with a DIFFERENT visible set per row: every row keeps about half of its visible devices and shows
    about a third of the hidden ones (KNOWN / OWNED move with it, as they do when a game goes on)."""
    rs = np.random.RandomState(seed)
    f = np.asarray(flags, np.uint8).copy()
    hide = rs.rand(*f.shape) < 0.5
    show = rs.rand(*f.shape) < 0.35
    vis_bits = np.uint8(S.F_KNOWN | S.F_OWNED)
    clear = np.uint8(0xFF ^ (S.F_KNOWN | S.F_OWNED | S.F_NYA))
    if role in (2, "attacker"):
        vis = ((f & S.F_KNOWN) != 0) & ((f & S.F_OWNED) != 0) & ((f & S.F_NYA) == 0)
        f = np.where(vis & hide, (f & clear) | np.uint8(S.F_KNOWN), f)
        f = np.where(~vis & show, (f & clear) | vis_bits, f)
    else:
        vis = ((f & S.F_NYA) == 0) & ((f & S.F_OWNED) == 0)
        f = np.where(vis & hide, (f & clear) | np.uint8(S.F_OWNED | S.F_KNOWN), f)
        f = np.where(~vis & show, (f & clear) | np.where(rs.rand(*f.shape) < 0.5, S.F_KNOWN, 0).astype(np.uint8), f)
    return f.astype(np.uint8)
