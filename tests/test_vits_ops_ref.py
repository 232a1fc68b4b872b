"""Pins tests/vits_ops_ref.py -- the fp64 references of the op-level VITS GPU tests -- to the oracle's WN / PosteriorEncoder /
ResidualCouplingBlock, which are themselves pinned to golden vectors of the real classes (tests/test_oracle_vits.py).  The pieces
composed the way the modules compose them must give the oracle's result to 1e-12 in fp64: the GPU tests' reference is then not a
second, unverified implementation."""
from collections import OrderedDict

import pytest
import torch
import torch.nn.functional as F

import vits_ops_ref as ref
from oracle import synth
from oracle import vocoder_oracle as vo

F64 = torch.float64
TIE = 1e-12


def _wn_by_pieces(sd, prefix, x, lens, n_layers, H, k, rate, g):
    """WN.forward modules/flow/modules.py:126-151 out of ref.wn_gate / ref.wn_accumulate / ref.sequence_mask"""
    cond = None
    if g is not None:
        wc, bc = vo.conv_params(sd, f"{prefix}.cond_layer", F64)
        cond = F.conv1d(g, wc, bc)                                   # [B, 2H * n_layers, 1]
    out = torch.full_like(x, float("nan"))                           # `first` must not read it
    for i in range(n_layers):
        d = rate**i
        w, b = vo.conv_params(sd, f"{prefix}.in_layers.{i}", F64)
        a = F.conv1d(x, w, b, dilation=d, padding=(k * d - d) // 2)
        acts = ref.wn_gate(a, cond[:, i * 2 * H:(i + 1) * 2 * H, 0] if cond is not None else None)
        w, b = vo.conv_params(sd, f"{prefix}.res_skip_layers.{i}", F64)
        x, out = ref.wn_accumulate(x, out, F.conv1d(acts, w, b), lens, first=(i == 0), last=(i == n_layers - 1))
    return ref.sequence_mask(out, lens)


@pytest.mark.parametrize("gin,n_layers,k,rate", [(0, 4, 5, 1), (8, 3, 3, 2), (8, 1, 5, 1)])
def test_gate_and_accumulate_compose_to_the_oracle_wn(gin, n_layers, k, rate):
    H, B, T = 16, 3, 41
    sd = synth.synth_state_dict(synth.wn_param_shapes(OrderedDict(), "enc", H, k, n_layers, gin), 99, g_gain=0.5)
    gen = torch.Generator().manual_seed(5)
    lens = torch.tensor([41, 17, 1])
    mask = ref.seq_mask(lens, B, T, F64)
    x = torch.randn(B, H, T, generator=gen, dtype=F64) * mask
    g = torch.randn(B, gin, 1, generator=gen, dtype=F64) if gin else None
    want = vo.wn_forward(sd, "enc", x, mask, n_layers, H, k, rate, F64, g=g)
    got = _wn_by_pieces(sd, "enc", x, lens, n_layers, H, k, rate, g)
    assert want.abs().max().item() > 0.1
    assert (got - want).abs().max().item() <= TIE


@pytest.mark.parametrize("gin", [0, 8])
def test_posterior_sample_is_the_oracle_z(gin):
    B, T, C = 3, 29, 8
    sd = synth.synth_state_dict(synth.posterior_encoder_param_shapes(20, C, 16, 3, gin_channels=gin), 2468, g_gain=0.5)
    gen = torch.Generator().manual_seed(7)
    y = torch.rand(B, 20, T, generator=gen, dtype=F64)
    lens = torch.tensor([29, 12, 1])
    noise = torch.randn(B, C, T, generator=gen, dtype=F64)
    g = torch.randn(B, gin, 1, generator=gen, dtype=F64) if gin else None
    z, m, logs, _ = vo.posterior_encoder_forward(sd, "", y, lens, noise, out_channels=C, hidden=16, n_layers=3, dtype=F64, g=g)
    assert logs.abs().max().item() > 0.01 and z.abs().max().item() > 0.1
    assert (ref.posterior_sample(torch.cat([m, logs], 1), noise, lens) - z).abs().max().item() <= TIE


@pytest.mark.parametrize("gin", [0, 8])
@pytest.mark.parametrize("reverse", [False, True])
def test_coupling_and_flip_compose_to_the_oracle_block(gin, reverse):
    B, T, C, H, n_layers, n_flows = 3, 33, 12, 16, 2, 4
    sd = synth.synth_state_dict(synth.coupling_block_param_shapes(C, H, n_layers, n_flows, gin_channels=gin), 1357, g_gain=0.5)
    gen = torch.Generator().manual_seed(9)
    lens = torch.tensor([33, 20, 2])
    mask = ref.seq_mask(lens, B, T, F64)
    x = torch.randn(B, C, T, generator=gen, dtype=F64) * mask
    g = torch.randn(B, gin, 1, generator=gen, dtype=F64) if gin else None
    want = vo.coupling_block_forward(sd, "", x, mask, reverse=reverse, channels=C, hidden=H, n_flows=n_flows, n_layers=n_layers, dtype=F64, g=g)
    got = x
    order = list(range(2 * n_flows))
    moved = 0.0
    for idx in (order[::-1] if reverse else order):
        if idx % 2:
            got = ref.flip_channels(got)
            continue
        p = f"flows.{idx}"
        w, b = vo.conv_params(sd, f"{p}.pre", F64)
        h = F.conv1d(got[:, :C // 2], w, b) * mask
        h = vo.wn_forward(sd, f"{p}.enc", h, mask, n_layers, H, 5, 1, F64, g=g)
        w, b = vo.conv_params(sd, f"{p}.post", F64)
        m = F.conv1d(h, w, b)
        moved = max(moved, (m * mask).abs().max().item())
        m = m.masked_fill(mask.expand_as(m) == 0, float("nan"))      # the kernel's contract: m is unspecified beyond the length
        got = ref.coupling_apply(got, m, lens, reverse)
    assert moved > 0.01                                              # the couplings do something with these weights
    assert (got - want).abs().max().item() <= TIE
