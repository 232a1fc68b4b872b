"""modules/encoder/token_encoder.py: ``TokenEmbedding``, the parameter ``word_embeddings.weight`` under the reference's name.  VALL-E reads the
table in place (``amp_embed_pos``, ``amp_embed_sum_c``)."""
import torch.nn as nn


class TokenEmbedding(nn.Module):
    def __init__(self, dim_model, vocab_size, dropout=0.0):
        super().__init__()
        self.dropout = nn.Dropout(p=dropout)
        self.word_embeddings = nn.Embedding(vocab_size, dim_model)

    @property
    def weight(self):
        return self.word_embeddings.weight
