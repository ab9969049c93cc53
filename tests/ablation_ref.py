"""Dense torch restatement of what ``OursLayer2`` adds (Ablation.py:140-205), for the tests:
its split intra core and the layer's BatchNorm tail.  Written in the closed form the kernels
use, not as the reference's masked softmax, so that tests/test_ablation_host.py can tie the
form to the reference's own outputs (tests/golden/ablations.npz) and the GPU tests can tie
the kernels to the form.
"""
import torch
import torch.nn.functional as F


def dense_split_core(el, er, h1, h2, mask, city, prov, src, keep_e=None, keep3=None,
                     keep4=None, p=0.0):
    """One head of Ablation.py:174-202 up to the BatchNorms: returns (u, v).

    The inter part is OursLayer3's (scores, row softmax over the mask, an empty row
    uniform, dropout).  The intra scores are constant along n, so each softmax row is
    1 / c on the c members of the source's group: for batch entry b with source s_b
      IntraNC_n = sum_{b: city(s_b) = city(n)} keep3[b, n] h2[s_b] / c3_b
                + sum_{b: prov(s_b) = prov(n)} keep4[b, n] h2[s_b] / c4_b
    (no dependence on a3 / a4).  keep_e (N, M), keep3 / keep4 (B, N): 0/1 keep masks,
    scaled by 1 / (1 - p) here."""
    e12 = F.leaky_relu(el[:, None] + er[None, :], 0.2)
    att = torch.softmax(torch.where(mask, e12, torch.full_like(e12, -9e15)), dim=1)
    if keep_e is not None:
        att = att * keep_e / (1 - p)
    hb = h2[src]
    m3 = (city[src][:, None] == city[None, :]).to(h2.dtype)  # (B, N)
    m4 = (prov[src][:, None] == prov[None, :]).to(h2.dtype)
    a3 = m3 / m3.sum(1, keepdim=True)
    a4 = m4 / m4.sum(1, keepdim=True)
    if keep3 is not None:
        a3 = a3 * keep3 / (1 - p)
        a4 = a4 * keep4 / (1 - p)
    u = att @ h1 + a3.t() @ hb + a4.t() @ hb
    v = att.t() @ h2
    return u, v


def bn_train(x, weight, bias, eps):
    """Training-mode BatchNorm1d of (rows, C): batch mean, biased variance."""
    mean = x.mean(0)
    var = x.var(0, unbiased=False)
    return (x - mean) / torch.sqrt(var + eps) * weight + bias


def bn_eval(x, weight, bias, mean, var, eps):
    return (x - mean) / torch.sqrt(var + eps) * weight + bias


def dense_layer_tail(u, v, bn_u, bn_v, eps=1e-5, slope=0.2, running=None):
    """Ablation.py:201-205 on the aggregates: elu(lrelu(bn2(u)) @ lrelu(bn1(v)).T).
    bn_u / bn_v: (weight, bias); running: ((mean_u, var_u), (mean_v, var_v)) for eval."""
    if running is None:
        uo = F.leaky_relu(bn_train(u, *bn_u, eps), slope)
        vo = F.leaky_relu(bn_train(v, *bn_v, eps), slope)
    else:
        uo = F.leaky_relu(bn_eval(u, *bn_u, *running[0], eps), slope)
        vo = F.leaky_relu(bn_eval(v, *bn_v, *running[1], eps), slope)
    return F.elu(uo @ vo.t())
