"""modules/norms/norm.py: ``LayerNorm`` and ``AdaptiveLayerNorm`` under the reference's parameter names, over the channel axis of the tree's
channel-first [B, C, T] tensors (``amp_layer_norm_c``).

``AdaptiveLayerNorm`` is ``weight * LN(x) + bias`` with ``weight | bias = project_layer(embedding)``.  In VALL-E the embedding is the one row
of a stage's ``nar_stage_embeddings``, so the pair depends on the stage alone: ``folded`` forms, on the host in fp64,

    gamma' = weight * norm.weight          beta' = weight * norm.bias + bias

once per (parameters, embedding, device) and the norm runs as ONE ``amp_layer_norm_c`` with that pair."""
import torch
import torch.nn as nn

from amphion_amd._handle import param_sig
from amphion_amd.modules.hip_ops import layer_norm_c


class LayerNorm(nn.Module):
    def __init__(self, normalized_shape, eps=1e-5, elementwise_affine=True, device=None, dtype=None):
        super().__init__()
        if isinstance(normalized_shape, int):
            normalized_shape = (normalized_shape,)
        self.normalized_shape = tuple(normalized_shape)
        if len(self.normalized_shape) != 1 or not elementwise_affine:
            raise NotImplementedError("LayerNorm: one normalised axis with an affine is what the HIP path covers")
        self.eps, self.elementwise_affine = eps, elementwise_affine
        self.weight = nn.Parameter(torch.ones(self.normalized_shape, device=device, dtype=dtype))
        self.bias = nn.Parameter(torch.zeros(self.normalized_shape, device=device, dtype=dtype))

    def affine(self, embedding=None):
        return self.weight.detach(), self.bias.detach()

    def forward_cf(self, x, embedding=None):
        """x [B, C, T] -> LN over C"""
        g, b = self.affine()
        return layer_norm_c(x, g, b, eps=self.eps)

    def extra_repr(self):
        return f"{self.normalized_shape}, eps={self.eps}, elementwise_affine={self.elementwise_affine}"


def fold_adaptive(project_weight, project_bias, norm_weight, norm_bias, embedding):
    """the host fold, fp64 -> (gamma', beta') fp32 on the host; embedding [1, d] or [d]"""
    d = norm_weight.numel()
    f = lambda t: t.detach().to("cpu", torch.float64)
    wb = f(embedding).reshape(1, d) @ f(project_weight).t() + f(project_bias)
    w, b = wb[0, :d], wb[0, d:]
    return (w * f(norm_weight)).float(), (w * f(norm_bias) + b).float()


class AdaptiveLayerNorm(nn.Module):
    def __init__(self, d_model, norm):
        super().__init__()
        self.project_layer = nn.Linear(d_model, 2 * d_model)
        self.norm = norm
        self.d_model = d_model
        self.eps = self.norm.eps
        self._folded = {}          # id(embedding) -> (signature, gamma', beta')

    def affine(self, embedding):
        """(gamma', beta') on the parameters' device for this embedding, rebuilt when a parameter or the embedding changes"""
        p, n = self.project_layer, self.norm
        if embedding is None or embedding.numel() != self.d_model:
            raise NotImplementedError("AdaptiveLayerNorm: the HIP path folds ONE embedding row per call (VALL-E's stage embedding)")
        dev = n.weight.device
        sig = param_sig((p.weight, p.bias, n.weight, n.bias, embedding), str(dev))
        hit = self._folded.get(id(embedding))
        if hit is None or hit[0] != sig:
            g, b = fold_adaptive(p.weight, p.bias, n.weight, n.bias, embedding)
            if len(self._folded) >= 16:
                self._folded.clear()
            hit = self._folded[id(embedding)] = (sig, g.to(dev), b.to(dev))
        return hit[1], hit[2]

    def forward_cf(self, x, embedding):
        g, b = self.affine(embedding)
        return layer_norm_c(x, g, b, eps=self.eps)
