"""The resident form of conv2's input gradient (convt2_resident_kernel, convt2.hpp:
W2^T held in LDS for a block's lifetime, three teams of four waves per block)
against the staging form (convt2_kernel), bit for bit.

The two forms run the same tiles in the same k order, sum a team's Gram in the
same tile and wave order into the same partial slot and publish max |d1| into the
same slots, so every output word is compared with torch.equal -- no tolerance.
"""
import ctypes

import pytest
import torch

from actorcritic import _lib

from test_gpu_kernels import alloc_acts, rand_params

pytestmark = pytest.mark.gpu

A, C3 = 4, 32
K_AMAX = 64 * 64  # kAmaxWords (common.hpp): 64 slots, 64 words apart
GRAM_SLOTS = 768  # convt2_gram_blocks' cap


def _prepared_net(lib, cuda, seed):
    params = rand_params(A, C3, cuda, seed=seed)
    prep = torch.empty(int(lib.acmi_conv_prep_bytes(C3)), dtype=torch.uint8, device=cuda)
    net = _lib.Net(A, C3, params.data_ptr(), prep.data_ptr())
    _lib.call('acmi_conv_prepare', ctypes.byref(net), _lib.ptr(prep), _lib.stream_handle())
    return params, prep, net


def _published_max(x, cuda):
    """max |x| as the dX chain's epilogues publish it: the float's bits in one slot"""
    words = torch.zeros(K_AMAX, dtype=torch.int32, device=cuda)
    words[0] = x.abs().max().view(torch.int32)
    return words


@pytest.mark.parametrize('B', [1, 37, 1000])
def test_resident_kernel_bit_identical_to_staging(lib, cuda, B):
    """acmi_debug_convt2 mode 2 (both launches on the resident kernel) against mode 0
    (the staging kernel): d1, every max |d1| slot word and the whole Gram partial
    buffer are equal.  B = 1: one ragged tile, two idle teams in the only block;
    B = 37: 29 tiles, the last ragged, a last block with an idle team, tiles that
    straddle images; B = 1000: 782 tiles > 768 teams, so 14 teams take two tiles and
    prefetch across the tile boundary.  d2a / d2b are seeded normal values of the
    size of a loss gradient (1 / B), the ReLU' mask words come from a forward pass
    (about half the bits set)."""
    params, prep, net = _prepared_net(lib, cuda, seed=21)
    g = torch.Generator().manual_seed(100 + B)
    obs = torch.randint(0, 256, (B, 84, 84, 4), generator=g, dtype=torch.uint8).to(cuda)
    t, acts = alloc_acts(B, A, C3, cuda, masks=True)
    _lib.call('acmi_forward', ctypes.byref(net), _lib.ptr(obs), 84 * 84 * 4, B, ctypes.byref(acts), 1,
              _lib.stream_handle())
    torch.cuda.synchronize()
    set_bits = sum(bin(w & 0xffffffff).count('1') for w in t['m1'].flatten()[:4000].tolist())
    assert 0.2 < set_bits / (32.0 * min(4000, B * 400)) < 0.8
    d2a = (torch.randn(B, 9, 9, 64, generator=g) / B).to(cuda)
    d2b = (torch.randn(B, 9, 9, 64, generator=g) / B).to(cuda)
    d2max_a, d2max_b = _published_max(d2a, cuda), _published_max(d2b, cuda)
    out = {}
    for mode in (0, 2):
        d1 = torch.zeros(B, 20, 20, 32, device=cuda)
        gram = torch.zeros(GRAM_SLOTS * 33 * 32, device=cuda)
        d1max = torch.zeros(K_AMAX, dtype=torch.int32, device=cuda)
        _lib.call('acmi_debug_convt2', ctypes.byref(net), mode, _lib.ptr(d2a), _lib.ptr(d2b), _lib.ptr(t['m1']),
                  _lib.ptr(d1), B, _lib.ptr(gram), _lib.ptr(d2max_a), _lib.ptr(d2max_b), _lib.ptr(d1max),
                  _lib.stream_handle())
        torch.cuda.synchronize()
        out[mode] = (d1, d1max, gram)
    d1, d1max, gram = out[0]
    assert d1.abs().max() > 0 and gram.abs().max() > 0
    assert d1max.max().view(torch.float32).item() == d1.abs().max().item()
    assert torch.equal(out[2][0], d1)
    assert torch.equal(out[2][1], d1max)
    assert torch.equal(out[2][2], gram)


@pytest.mark.parametrize('masks', [True, False], ids=['mask-words', 'f32-activations'])
def test_backward_and_output_stats_bit_identical_across_forms(lib, cuda, masks):
    """acmi_backward + acmi_kfac_output_stats at B = 1000 with the resident form
    forced off and then on: gradients, A and G factors and the loss chain's d1 are
    equal.  The switch is acmi_debug_convt2_form (0 = staging, 1 = resident; the
    previous setting is put back), so the test does not depend on where the
    batch-size thresholds of convt2.hpp stand.  masks: ReLU' from the mask words or
    from the f32 activations -- the kernels' two MASK instantiations."""
    B = 1000
    params, prep, net = _prepared_net(lib, cuda, seed=22)
    g = torch.Generator().manual_seed(23)
    obs = torch.randint(0, 256, (B, 84, 84, 4), generator=g, dtype=torch.uint8).to(cuda)
    t, acts = alloc_acts(B, A, C3, cuda, masks=masks)
    _lib.call('acmi_forward', ctypes.byref(net), _lib.ptr(obs), 84 * 84 * 4, B, ctypes.byref(acts), 1,
              _lib.stream_handle())
    ldh = 8
    dhead = torch.zeros(B, ldh)
    dhead[:, :A + 1] = torch.randn(B, A + 1, generator=g) / B
    dhead = dhead.to(cuda)
    z = lambda *s: torch.zeros(*s, dtype=torch.float32, device=cuda)
    so = (ctypes.c_int64 * 11)()
    tot = ctypes.c_int64()
    _lib.call('acmi_kfac_layout', A, C3, None, None, so, ctypes.byref(tot))
    ws = z(lib.acmi_backward_ws_floats(B, A, C3))
    out = {}
    prev = lib.acmi_debug_convt2_form(-1)
    try:
        for form in (0, 1):
            lib.acmi_debug_convt2_form(form)
            d = [z(B, 20, 20, 32), z(B, 9, 9, 64), z(B, 7, 7, C3), z(B, 512)]
            bwd = _lib.Bwd(*[x.data_ptr() for x in d], dhead.data_ptr(), ldh)
            grads, astat, gstat = z(params.numel()), z(tot.value), z(tot.value)
            _lib.call('acmi_backward', ctypes.byref(net), _lib.ptr(obs), 84 * 84 * 4, B, ctypes.byref(acts),
                      ctypes.byref(bwd), _lib.ptr(grads), _lib.ptr(astat), _lib.ptr(ws), ws.numel(),
                      _lib.stream_handle())
            torch.cuda.synchronize()
            d1 = d[0].clone()
            _lib.call('acmi_kfac_output_stats', ctypes.byref(net), B, ctypes.byref(acts), ctypes.byref(bwd),
                      7, 0, 3, _lib.ptr(gstat), _lib.ptr(ws), ws.numel(), _lib.stream_handle())
            torch.cuda.synchronize()
            out[form] = (grads, astat, gstat, d1)
    finally:
        lib.acmi_debug_convt2_form(prev)
    o0 = so[5]
    assert out[0][2][o0:o0 + 32 * 32].abs().max() > 0 and out[0][3].abs().max() > 0
    for name, a, b in zip(('grads', 'a_stats', 'g_stats', 'd1'), out[0], out[1]):
        assert torch.equal(a, b), name
