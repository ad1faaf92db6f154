"""ops.mla_attention takes the scheduler's max_query_len hint on every
backend; the CPU reference has no use for it and must ignore it."""

import torch

import vllm_amd.ops as ops


def test_mla_attention_accepts_max_query_len_on_cpu():
    torch.manual_seed(0)
    Hq, lora, rope, bs = 4, 64, 16, 16
    kv = torch.randn(5, bs, lora + rope)
    bt = torch.tensor([[3, 1], [2, 4]], dtype=torch.int32)
    qsl = torch.tensor([0, 1, 8], dtype=torch.int32)
    seq_lens = torch.tensor([20, 7], dtype=torch.int32)
    q_nope = torch.randn(8, Hq, lora)
    q_pe = torch.randn(8, Hq, rope)
    args = (q_nope, q_pe, kv, bt, qsl, seq_lens, 0.1)
    plain = ops.mla_attention(*args, num_decodes=1, max_seq_len=20)
    hinted = ops.mla_attention(*args, num_decodes=1, max_seq_len=20,
                               max_query_len=7)
    torch.testing.assert_close(hinted, plain, rtol=0, atol=0)
