"""The streamed window attention on the host: the argument checks of dlmcq_window_attention_stream_f32 on placeholder pointers (nothing
is launched) - window_attention_args with the token limit 256 -, the 64-token entries' refusal as it was, and the Python views."""
import pytest
import torch

from dlmc import _native as N
from dlmc.quantization.scalar import kernels as K
from test_transformer_host import EINVAL
from test_window_attention_host import ANSWERS, _wa

ENTRY = "dlmcq_window_attention_stream_f32"      # (every answer of the 64-token entry but t = 65's, and the new limit's)
STREAM = dict({k: v for k, v in ANSWERS.items() if k != "t_65"}, t_65_b_0=(dict(t=65, b=0), 0), t_256_b_0=(dict(t=256, b=0), 0),
              t_257=(dict(t=257), EINVAL), row_stride_below_t=(dict(t=144, bias_s=(144 * 140, 140)), EINVAL))


@pytest.mark.parametrize("name", sorted(STREAM))
def test_return_codes_need_no_gpu(name):
    kw, rc = STREAM[name]
    assert _wa(entry=ENTRY, **kw) == rc and N.SIGNATURES[ENTRY] == N.SIGNATURES["dlmcq_window_attention_f32"]


def test_the_64_token_entries_and_views_are_as_they_were():
    qkv = lambda t, d=32: [torch.zeros(1, 2, t, d)] * 3  # noqa: E731
    assert _wa(t=65) == EINVAL and _wa(t=65, entry="dlmcq_window_attention_f16") == EINVAL and (K.WINDOW_TOKENS, K.WINDOW_STREAM_TOKENS) == (64, 256)
    assert K.window_stream_views(*qkv(256)) and K.window_stream_views(*qkv(1)) and not K.window_stream_views(*qkv(257)) and not K.window_stream_views(*qkv(144, 48))
    assert K.window_attention_views(*qkv(64)) and not K.window_attention_views(*qkv(65))
