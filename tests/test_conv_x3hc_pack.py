"""The weight operands of x3hc (csrc/kernels/halo_x3c.hip) as the planner packs them: the 3x3 planes round-trip to
the fp32 weights with zero padded K, and the 1x1 operand holds every 3x3 channel where the kernel's lanes read it."""
from __future__ import annotations

import pytest
import torch

from inference_arena_amd.engine.planner import pack_conv_weight_x3, pack_pw_weight_x3


def _planes(raw: bytes, *shape):
    return torch.frombuffer(bytearray(raw), dtype=torch.bfloat16).reshape(*shape).float()


@pytest.mark.parametrize("cin", [80, 64])
def test_conv_planes_round_trip_with_zero_padded_k(cin):
    w = torch.randn(80, cin, 3, 3, generator=torch.Generator().manual_seed(cin))
    nc = (cin + 31) // 32
    p = _planes(pack_conv_weight_x3(w), 9, nc, 80, 3, 32)  # [tap][chunk][row][h | m | l][k]: one stage = [80][96]
    k = p.sum(3).permute(2, 0, 1, 3).reshape(80, 9, nc * 32)  # h + m + l, exact in fp32
    assert torch.equal(k[:, :, :cin], w.permute(0, 2, 3, 1).reshape(80, 9, cin))
    assert torch.all(p.permute(2, 0, 3, 1, 4).reshape(80, 9, 3, nc * 32)[..., cin:] == 0)


@pytest.mark.parametrize("c2", [80, 64])
def test_pw_planes_hold_each_lanes_four_channels_in_a_row(c2):
    w2 = torch.randn(c2, 80, 1, 1, generator=torch.Generator().manual_seed(c2))
    p = _planes(pack_pw_weight_x3(w2, 96), -1, 3, 96).sum(1)  # [rows][96]
    for j in range(5):  # 3x3 fragment j, lane quarter q: channels 16 j + 4 q + {0..3} at columns 16 j + 8 (q & 1) + 4 (q >> 1)
        for q in range(4):
            c0, k0 = 16 * j + 4 * q, 16 * j + 8 * (q & 1) + 4 * (q >> 1)
            assert torch.equal(p[:c2, k0:k0 + 4], w2[:, c0:c0 + 4, 0, 0])
    assert torch.all(p[c2:] == 0) and torch.all(p[:, 80:] == 0)
