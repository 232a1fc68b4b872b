"""modules/transformer/position_embedding.py: ``SinePositionalEmbedding``, the parameter ``alpha`` under the reference's name and the table
``pe`` built with the reference's own formula (a plain attribute there too: not in the ``state_dict``).  VALL-E adds the rows on the device
(``amp_embed_pos`` from a running position)."""
import math

import torch
import torch.nn as nn


def sine_table(rows, dim_model):
    """position_embedding.py:43-48, fp32 on the host: sin on the even channels, cos on the odd ones"""
    pe = torch.zeros(rows, dim_model)
    position = torch.arange(0, rows, dtype=torch.float32).unsqueeze(1)
    div_term = torch.exp(torch.arange(0, dim_model, 2, dtype=torch.float32) * -(math.log(10000.0) / dim_model))
    pe[:, 0::2] = torch.sin(position * div_term)
    pe[:, 1::2] = torch.cos(position * div_term)
    return pe


class SinePositionalEmbedding(nn.Module):
    def __init__(self, dim_model, dropout=0.0, scale=False, alpha=False):
        super().__init__()
        self.dim_model = dim_model
        self.x_scale = math.sqrt(dim_model) if scale else 1.0
        self.alpha = nn.Parameter(torch.ones(1), requires_grad=alpha)
        self.dropout = nn.Dropout(p=dropout)
        self.reverse = False
        self._tables = {}          # device -> pe [rows, dim_model]

    def table(self, rows, device):
        """pe [>= rows, dim_model] on ``device``: 4000 rows as the reference starts with, more when a sequence needs them; uploaded once"""
        key = str(device)
        t = self._tables.get(key)
        if t is None or t.shape[0] < rows:
            t = self._tables[key] = sine_table(max(4000, int(rows)), self.dim_model).to(device)
        return t
