"""CPU: the tile-route plan of the ten fused ops that keep a workgroup's tile in the LDS or, past 160 KiB, in a per-workgroup slice of
the workspace (csrc/tile_route.h): what their *_workspace_bytes / *_bwd_supported entry points answer.  Host arithmetic only — nothing
is launched.

Every non-zero expectation below is a literal number: the reply of the library as built from the commit BEFORE tile_route.h existed
(each op then carried its own copy of the limits and of the slice arithmetic), not a value computed by the code under test.  The
shapes are the smallest (in the one size that is varied) at which that library answered non-zero; the shape one step below it is the
LDS-route case and answers 0.  A workspace holds one slice per workgroup, never one per sample: the reply does not depend on the batch."""
import pytest

from deepctr_amd import ops

BATCHES = (1, 5, 70000)
CONV, POOL = [(7, 1, 14)], [("kmax", 3)]

# name: (reply(batch, n), the smallest n on the workspace route, the bytes there); dim = 64 where the op has one
THRESHOLDS = {
    "interacting": (lambda B, F: ops.interacting_workspace_bytes(B, F, 64, 1, 8, 2, True, True), 299, 41988096),
    "interacting_bwd": (lambda B, F: ops.interacting_bwd_workspace_bytes(B, F, 64, 1, 8, 2, True), 81, 42348544),
    "bilinear": (lambda B, F: ops.senet_bilinear_workspace_bytes(B, F, 64, "all", 0, 2), 11, 43409408),
    "bilinear_bwd": (lambda B, F: ops.senet_bilinear_bwd_workspace_bytes(B, F, 64, "all", "model", 2), 7, 45121536),
    "fieldpair-fefm": (lambda B, F: ops.fieldpair_workspace_bytes(B, F, 64, "fefm"), 38, 42614784),
    "fieldpair-fwfm": (lambda B, F: ops.fieldpair_workspace_bytes(B, F, 64, "fwfm"), 41, 42991616),
    "fieldpair_bwd-fefm": (lambda B, F: ops.fieldpair_bwd_workspace_bytes(B, F, 64, "fefm"), 35, 42393600),
    "fieldpair_bwd-fwfm": (lambda B, F: ops.fieldpair_bwd_workspace_bytes(B, F, 64, "fwfm"), 39, 42512384),
    "transformer": (lambda B, T: ops.transformer_workspace_bytes(B, T, 64, 1), 69, 42102784),
    "gru": (lambda B, E: ops.gru_workspace_bytes(B, 4, E), 497, 41959424),
    "lstm": (lambda B, T: ops.bilstm_workspace_bytes(B, T, 64, 64, 1), 11, 43352064),
    "fieldconv": (lambda B, F: ops.field_conv_workspace_bytes(B, F, 64, CONV, POOL), 168, 42041344),
}


@pytest.mark.parametrize("name", sorted(THRESHOLDS))
def test_workspace_bytes_at_the_lds_limit(name):
    reply, n, nbytes = THRESHOLDS[name]
    for B in BATCHES:
        assert reply(B, n - 1) == 0                 # the LDS route
        assert reply(B, n) == nbytes                # 256 slices of one tile, whatever the batch
    assert nbytes % (256 * 16) == 0 and nbytes // 256 > 160 * 1024


def test_bwd_supported_on_both_routes():
    for F in (80, 81):
        assert ops.interacting_bwd_supported(F, 64, 1, 8, 2, True)
    for F in (6, 7):
        assert ops.senet_bilinear_bwd_supported(F, 64, "all", "model", 2)
    for F, kind in ((34, "fefm"), (35, "fefm"), (38, "fwfm"), (39, "fwfm")):
        assert ops.fieldpair_bwd_supported(F, 64, kind)
    # refused for another reason than the tile's size: no workspace is asked for either
    assert not ops.interacting_bwd_supported(26, 16, 33, 8, 2, True)                    # more layers than one launch takes
    assert ops.interacting_bwd_workspace_bytes(5, 26, 16, 33, 8, 2, True) == 0


def test_fewer_slices_for_larger_tiles():
    """Past 1 MiB per tile the 256 MiB cap leaves fewer than 256 slices; a tile past the cap still gets one."""
    for B in BATCHES:
        assert ops.fieldpair_workspace_bytes(B, 200, 64, "fefm") == 212484096           # (the shape of tests/test_fefm_cpu.py)
        assert ops.fieldpair_workspace_bytes(B, 200, 256, "fefm") == 266296896
        assert ops.fieldpair_bwd_workspace_bytes(B, 200, 256, "fefm") == 267222240
        assert ops.fieldpair_bwd_workspace_bytes(B, 30000, 16, "fwfm") == 3630840064    # one slice
        assert ops.senet_bilinear_workspace_bytes(B, 200, 256, "all", 0, 66) == 260353600
        assert ops.senet_bilinear_bwd_workspace_bytes(B, 200, 256, "all", "model", 66) == 263580800
        assert ops.interacting_workspace_bytes(B, 2000, 160, 1, 8, 2, True, True) == 267264000
        assert ops.interacting_bwd_workspace_bytes(B, 2000, 160, 1, 8, 2, True) == 268164480
        assert ops.transformer_workspace_bytes(B, 4096, 160, 1) == 256216064
        assert ops.gru_workspace_bytes(B, 4, 4096) == 267608832
        assert ops.bilstm_workspace_bytes(B, 512, 64, 64, 1) == 268416000
        assert ops.field_conv_workspace_bytes(B, 4096, 64, CONV, POOL) == 267552256
    assert ops.fieldpair_bwd_supported(30000, 16, "fwfm")


def test_forced_workspace_route_of_a_tile_that_fits_the_lds():
    """transformer, bilstm and field_conv may be told to take the workspace route: 256 slices of a small tile."""
    for B in BATCHES:
        assert ops.transformer_workspace_bytes(B, 4, 8, 1, route="general") == 3133440
        assert ops.bilstm_workspace_bytes(B, 4, 8, 8, 1, route="workspace") == 5537792
        assert ops.field_conv_workspace_bytes(B, 8, 4, [(3, 1, 2)], POOL, route="workspace") == 1146880
        assert ops.transformer_workspace_bytes(B, 4, 8, 1) == 0
        assert ops.bilstm_workspace_bytes(B, 4, 8, 8, 1) == 0
        assert ops.field_conv_workspace_bytes(B, 8, 4, [(3, 1, 2)], POOL) == 0
