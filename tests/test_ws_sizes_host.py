"""CPU test of the size functions the callers allocate by: acmi_backward_ws_floats,
acmi_forward_ws_floats and acmi_conv_prep_bytes return exactly the values recorded in
tests/golden/ws_sizes.json (written from a build that predates csrc/backward.hpp's
prepared-buffer and workspace views), and the launch planners' self-check passes.
A layout section moved or a sizing term dropped shows here before any launch does."""
import json
import os

HERE = os.path.dirname(os.path.abspath(__file__))


def _golden():
    with open(os.path.join(HERE, 'golden', 'ws_sizes.json')) as f:
        return json.load(f)


def test_workspace_and_prep_sizes_match_the_recorded_values(lib):
    g = _golden()
    Bs, As, C3s = g['B'], g['A'], g['C3']
    assert Bs == [1, 2, 17, 32, 63, 64, 65, 129, 512, 640, 2560, 10240, 20480]
    assert As == [1, 4, 18, 31, 32, 33, 63, 64]
    assert C3s == [32, 64]
    assert len(g['backward_ws_floats']) == len(Bs) * len(As) * len(C3s)
    got = [int(lib.acmi_backward_ws_floats(B, A, C3)) for B in Bs for A in As for C3 in C3s]
    assert got == g['backward_ws_floats']
    assert [int(lib.acmi_forward_ws_floats(B)) for B in Bs] == g['forward_ws_floats']
    assert [int(lib.acmi_conv_prep_bytes(C3)) for C3 in C3s] == g['conv_prep_bytes']


def test_launch_planners_self_check(lib):
    assert lib.acmi_selftest_plans(4096) == 0
