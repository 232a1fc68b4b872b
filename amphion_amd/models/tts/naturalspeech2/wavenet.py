"""models/tts/naturalspeech2/wavenet.py on the HIP kernels, eval mode, ``x_mask = None`` (what the reference's inference passes).

A solver runs this network 200 - 500 times on one condition, so everything that does not depend on x is formed ONCE per utterance
(``WaveNet.prepare``):

    cond_ln                                   ``amp_layer_norm_c``
    cterm of every layer                      ONE stacked GEMM [L * 2H, H] on cond_ln(cond) (``cond_proj`` with its bias); chunked over layers
                                              so that a chunk stays under ``CTERM_CHUNK_BYTES``
    k | v of the speaker queries              ONE stacked GEMM [A * 2H, H] for the A layers with cross-attention
    dconst [n_times, L, H]                    sinusoidal embedding (host, fp32) -> ``mlp`` (two GEMMs with the step axis as columns, Mish in
                                              torch) -> ONE stacked ``diffusion_proj`` GEMM [L * H, H]

and a step (``WaveNet.step``) is: ``in_proj`` with ReLU on store; per layer with cross-attention ``y = x + dconst`` (one add), LayerNorm, the
q GEMM, ``amp_cross_attention`` over the 32 query tokens, ONE GEMM H -> 4H that is ``out_proj`` folded into ``film.gain | film.bias`` on the
host in fp64 (``fold_film``; the exact-fp32 route keeps the two GEMMs apart); then the layer op (``amp_ns2_layer_*``, two launches, x updated in
place, the skip sum accumulated in place); the tail is one scale by 1 / sqrt(L), ``skip_proj`` with ReLU on store and ``out_proj``.

Parameters and ``state_dict`` keys are the reference's."""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from amphion_amd import _lib
from amphion_amd._handle import param_sig
from amphion_amd.models.codec.amphion_codec.vocos import _PwHandle
from amphion_amd.models.vc.flow_matching_transformer.llama_nar import _pw
from amphion_amd.models.vocoders.gan.generator._engine import ConvParams
from amphion_amd.modules.hip_ops import HipConv1d, Ns2Layer, _workspace, cross_attention, layer_norm_c
from amphion_amd.modules.naturalpseech2.transformers import _check_mha, _eval_only, _Rows, _RowsHandle, mha_rows, stacked_kv_rows

CTERM_CHUNK_BYTES = 256 << 20


def fold_film(gain_w, gain_b, bias_w, bias_b, out_w, out_b):
    """``film.gain | film.bias`` applied to ``out_proj(a)`` as ONE affine map of a, formed in fp64: W = [Wg; Wb] Wo [4H, H] and
    b = [Wg; Wb] bo + [bg; bb] [4H] -> fp32"""
    wgb = torch.cat((gain_w, bias_w), 0).detach().double().cpu()
    bgb = torch.cat((gain_b, bias_b), 0).detach().double().cpu()
    wo, bo = out_w.detach().double().cpu(), out_b.detach().double().cpu()
    return (wgb @ wo).float(), (wgb @ bo + bgb).float()


class Mish(nn.Module):
    def forward(self, x):
        return x * torch.tanh(nn.functional.softplus(x))


class FiLM(nn.Module):
    """parameters only: the layer op applies ``x * gain + bias`` between the conv and the gate"""

    def __init__(self, in_dim, cond_dim):
        super().__init__()
        self.gain = nn.Linear(cond_dim, in_dim)
        self.bias = nn.Linear(cond_dim, in_dim)
        nn.init.xavier_uniform_(self.gain.weight)
        nn.init.constant_(self.gain.bias, 1)
        nn.init.xavier_uniform_(self.bias.weight)
        nn.init.constant_(self.bias.bias, 0)


class SinusoidalPosEmb(nn.Module):
    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def forward(self, x):
        half_dim = self.dim // 2
        emb = math.log(10000) / (half_dim - 1)
        emb = torch.exp(torch.arange(half_dim, device=x.device) * -emb)
        emb = x[:, None] * emb[None, :]
        return torch.cat((emb.sin(), emb.cos()), dim=-1)


class ResidualBlock(nn.Module):
    def __init__(self, hidden_dim, attn_head, dilation, drop_out, has_cattn=False):
        super().__init__()
        self.hidden_dim, self.dilation, self.has_cattn, self.attn_head, self.drop_out = hidden_dim, dilation, has_cattn, attn_head, drop_out
        self.dilated_conv = ConvParams(hidden_dim, 2 * hidden_dim, 3, padding=dilation, dilation=dilation, weight_norm=False)
        self.diffusion_proj = nn.Linear(hidden_dim, hidden_dim)
        self.cond_proj = ConvParams(hidden_dim, hidden_dim * 2, 1, weight_norm=False)
        self.out_proj = ConvParams(hidden_dim, hidden_dim * 2, 1, weight_norm=False)
        if has_cattn:
            self.attn = nn.MultiheadAttention(hidden_dim, attn_head, 0.1, batch_first=True)
            self.film = FiLM(hidden_dim * 2, hidden_dim)
            self.ln = nn.LayerNorm(hidden_dim)
            self._q, self._o, self._film = _RowsHandle(), _PwHandle(), _RowsHandle()
            self._fold_sig, self._fold, self._film_rows = None, None, None
        self.dropout = nn.Dropout(drop_out)
        self._op = Ns2Layer(hidden_dim, dilation)

    def _film_tensor(self, att):
        """att [B, H, T]: the attention's heads before out_proj -> gain | bias [B, 4H, T]"""
        f = self.film
        if _lib.get_precision() == "f32":
            a = _pw(self._o, self.attn.out_proj, att)
            if self._film_rows is None or self._film_rows[0] != param_sig((f.gain.weight, f.gain.bias, f.bias.weight, f.bias.bias)):
                rows = _Rows(torch.cat((f.gain.weight.detach(), f.bias.weight.detach()), 0), torch.cat((f.gain.bias.detach(), f.bias.bias.detach()), 0),
                             (f.gain.weight, f.gain.bias, f.bias.weight, f.bias.bias))
                self._film_rows = (param_sig(rows.tensors), rows)
            return _pw(self._film, self._film_rows[1], a)
        tensors = (f.gain.weight, f.gain.bias, f.bias.weight, f.bias.bias, self.attn.out_proj.weight, self.attn.out_proj.bias)
        sig = param_sig(tensors)
        if sig != self._fold_sig:
            w, b = fold_film(f.gain.weight, f.gain.bias, f.bias.weight, f.bias.bias, self.attn.out_proj.weight, self.attn.out_proj.bias)
            self._fold, self._fold_sig = _Rows(w, b, tensors), sig
        return _pw(self._film, self._fold, att)

    def film_of(self, x, dconst, k, v):
        """the cross-attention branch of a layer that has one: x [B, H, T], dconst [H], k / v [B, H, Q] (row blocks of the stacked speaker
        GEMM) -> gain | bias [B, 4H, T]"""
        y = x + dconst[None, :, None]
        y = layer_norm_c(y, self.ln.weight.detach(), self.ln.bias.detach(), eps=self.ln.eps)
        q = _pw(self._q, mha_rows(self.attn, 0, 1), y)
        return self._film_tensor(cross_attention(q, k, v, self.attn_head))

    def op_handle(self, device):
        return self._op.handle(self.dilated_conv.weight, self.dilated_conv.bias, self.out_proj.weight, self.out_proj.bias, device)

    def forward(self, x, x_mask, cond, diffusion_step, spk_query_emb):
        raise NotImplementedError("ResidualBlock.forward: the HIP path runs a layer through WaveNet.prepare / WaveNet.step (the step-invariant "
                                  "terms of all layers come from stacked GEMMs)")


class WaveNet(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.cfg = cfg
        self.in_dim, self.hidden_dim, self.out_dim = cfg.input_size, cfg.hidden_size, cfg.out_size
        self.num_layers, self.cross_attn_per_layer = cfg.num_layers, cfg.cross_attn_per_layer
        self.dilation_cycle, self.attn_head, self.drop_out = cfg.dilation_cycle, cfg.attn_head, cfg.drop_out
        H = self.hidden_dim
        self.in_proj = HipConv1d(self.in_dim, H, 1, weight_norm=False)
        self.diffusion_embedding = SinusoidalPosEmb(H)
        self.mlp = nn.Sequential(nn.Linear(H, H * 4), Mish(), nn.Linear(H * 4, H))
        self.cond_ln = nn.LayerNorm(H)
        self.layers = nn.ModuleList([ResidualBlock(H, self.attn_head, 2 ** (i % self.dilation_cycle), self.drop_out,
                                                   has_cattn=(i % self.cross_attn_per_layer == 0)) for i in range(self.num_layers)])
        self.skip_proj = HipConv1d(H, H, 1, weight_norm=False)
        self.out_proj = HipConv1d(H, self.out_dim, 1, weight_norm=False)
        nn.init.zeros_(self.out_proj.weight)
        self._mlp0, self._mlp2, self._dproj, self._kv = _PwHandle(), _PwHandle(), _RowsHandle(), _RowsHandle()
        self._cterm = {}       # layers per chunk -> [_RowsHandle]
        self._stacks_sig, self._stacks = None, None

    def _stacked(self):
        """the re-stacked weights of the once-per-utterance GEMMs, rebuilt when a parameter they are cut from changes"""
        tensors = [t for l in self.layers for t in (l.cond_proj.weight, l.cond_proj.bias, l.diffusion_proj.weight, l.diffusion_proj.bias)]
        attns = [l.attn for l in self.layers if l.has_cattn]
        tensors += [t for a in attns for t in (a.in_proj_weight, a.in_proj_bias)]
        sig = param_sig(tensors)
        if sig != self._stacks_sig:
            H = self.hidden_dim
            dproj = _Rows(torch.cat([l.diffusion_proj.weight.detach() for l in self.layers], 0),
                          torch.cat([l.diffusion_proj.bias.detach() for l in self.layers], 0),
                          tuple(t for l in self.layers for t in (l.diffusion_proj.weight, l.diffusion_proj.bias)))
            self._stacks = dict(dproj=dproj, kv=stacked_kv_rows(attns) if attns else None, cterm={})
            self._stacks_sig = sig
            self._cterm = {}
        return self._stacks

    def _cterm_rows(self, per):
        st = self._stacked()
        if per not in st["cterm"]:
            H, rows = self.hidden_dim, []
            for l0 in range(0, self.num_layers, per):
                ls = self.layers[l0:l0 + per]
                rows.append(_Rows(torch.cat([l.cond_proj.weight.detach().reshape(2 * H, H) for l in ls], 0), torch.cat([l.cond_proj.bias.detach() for l in ls], 0),
                                  tuple(t for l in ls for t in (l.cond_proj.weight, l.cond_proj.bias))))
            st["cterm"][per] = rows
            self._cterm[per] = [_RowsHandle() for _ in rows]
        return st["cterm"][per], self._cterm[per]

    def prepare(self, cond, spk_query_emb, times):
        """cond [B, H, T] channel-first (the prior's output), spk_query_emb [B, H, Q] channel-first, times: the step times as Python floats
        holding fp32 values, in the order the solver asks for them -> the state ``step`` reads"""
        _eval_only(self, "WaveNet")
        B, H, T = cond.shape
        dev = cond.device
        st = self._stacked()
        c = layer_norm_c(cond, self.cond_ln.weight.detach(), self.cond_ln.bias.detach(), eps=self.cond_ln.eps)
        per = max(1, min(self.num_layers, CTERM_CHUNK_BYTES // (B * 2 * H * T * 4)))
        rows, handles = self._cterm_rows(per)
        cterm = [_pw(h, r, c) for r, h in zip(rows, handles)]                    # each [B, per * 2H, T]
        kv = _pw(self._kv, st["kv"], spk_query_emb) if st["kv"] is not None else None
        # the step embedding of every time at once: sinusoidal on the host in fp32 as SinusoidalPosEmb forms it, steps as columns from there
        t = torch.tensor(list(times), dtype=torch.float32)
        e = self.diffusion_embedding(t).t().contiguous()[None].to(dev)           # [1, H, n]
        h = _pw(self._mlp0, self.mlp[0], e)
        h = h * torch.tanh(nn.functional.softplus(h))
        e = _pw(self._mlp2, self.mlp[2], h)
        d = _pw(self._dproj, st["dproj"], e)                                     # [1, L * H, n]
        dconst = d[0].t().contiguous().view(len(t), self.num_layers, H)          # [n, L, H]
        # what a step hands to amp_ns2_layer_forward, resolved once: the layers' handles, each layer's cterm row block (address and batch
        # stride), the attention layers' k / v row blocks, the workspace
        handles = [layer.op_handle(dev) for layer in self.layers]
        for layer in self.layers:
            if layer.has_cattn:
                _check_mha(layer.attn, "ResidualBlock")
        cptr, cbs = [], []
        for i in range(self.num_layers):
            ct = cterm[i // per]
            cptr.append(ct.data_ptr() + (i % per) * 2 * H * T * 4)
            cbs.append(ct.shape[1] * T)
        n_attn = sum(1 for layer in self.layers if layer.has_cattn)
        kvs = [(kv[:, 2 * H * a:2 * H * a + H], kv[:, 2 * H * a + H:2 * H * (a + 1)]) for a in range(n_attn)]
        ws_bytes = _lib.lib().amp_ns2_layer_workspace_bytes(handles[0], B, T)
        return dict(cterm=cterm, per=per, kv=kv, kvs=kvs, dconst=dconst, B=B, T=T, handles=handles, cptr=cptr, cbs=cbs, ws=_workspace(dev, ws_bytes),
                    ws_bytes=ws_bytes)

    def step(self, state, x, index):
        """x [B, latent, T], index: which of ``times`` -> [B, latent, T]"""
        H, L = self.hidden_dim, self.num_layers
        if tuple(x.shape) != (state["B"], self.in_dim, state["T"]):
            raise ValueError(f"WaveNet.step: expected x {(state['B'], self.in_dim, state['T'])} as prepared, got {tuple(x.shape)}")
        h = self.in_proj(x, slope_out=0.0)
        skip = torch.empty_like(h)
        B, T = state["B"], state["T"]
        hp, sp, wp, wb = h.data_ptr(), skip.data_ptr(), state["ws"].data_ptr(), state["ws_bytes"]
        dconst = state["dconst"]
        index = int(index)
        if not 0 <= index < dconst.shape[0]:
            raise IndexError(f"WaveNet.step: step time {index} of {dconst.shape[0]}")
        if any(layer._op._cache.handle is not hd for layer, hd in zip(self.layers, state["handles"])):
            raise RuntimeError("WaveNet.step: a parameter, the device or the precision changed since prepare(): prepare again")
        drow, dptr = dconst[index], dconst.data_ptr() + index * L * H * 4
        handles, cptr, cbs, kvs = state["handles"], state["cptr"], state["cbs"], state["kvs"]
        forward, stream = _lib.lib().amp_ns2_layer_forward, _lib.current_stream_ptr(h.device)
        a = 0
        for i, layer in enumerate(self.layers):
            film = None
            if layer.has_cattn:
                film = layer.film_of(h, drow[i], *kvs[a])
                a += 1
            # x is updated in place and the skip sum accumulates in place (no skip_in in the first layer); every argument was formed above
            # from tensors this module owns, at the shapes prepare() was given
            rc = forward(handles[i], hp, dptr + i * H * 4, 0, cptr[i], cbs[i], None if film is None else film.data_ptr(), sp if i else None, B, T, hp, sp,
                         wp, wb, stream)
            if rc < 0:
                _lib.check(rc)
        skip.mul_(1.0 / math.sqrt(self.num_layers))
        return self.out_proj(self.skip_proj(skip, slope_out=0.0))

    def forward(self, x, x_mask, cond, diffusion_step, spk_query_emb):
        """x [B, latent, T]; x_mask None; cond [B, T, H]; diffusion_step [B], ONE time for the whole batch (as every solver of the reference
        passes it; read on the host); spk_query_emb [B, Q, H] -> [B, latent, T]"""
        if x_mask is not None:
            raise NotImplementedError("WaveNet: x_mask is the training path; the reference's inference passes None")
        x = _lib.require_device_tensor(x, "WaveNet input")
        t = diffusion_step.detach().float().cpu()
        if t.numel() > 1 and not bool((t == t[0]).all()):
            raise NotImplementedError("WaveNet: one step time per item (training's draw) is not on the HIP path")
        with _lib.on_device(x.device):
            state = self.prepare(cond.transpose(1, 2).contiguous(), spk_query_emb.transpose(1, 2).contiguous(), [float(t.reshape(-1)[0])])
            return self.step(state, x, 0)
