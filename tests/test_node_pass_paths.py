"""Launcher choices of the node-side passes that are host logic (no GPU): which Gate kernel e3k_gate_fwd / e3k_gate_bwd pick
(``e3k_gate_path``) and the row tile of the radial MLP's hidden chain (``e3k_mlp_tile_rows``).  tests/test_gpu_node_passes.py runs
every form these choose between against float64."""
import pytest

C2 = 1.6791767923989418
LAYER = [(0, 0, 0, 0, 64, 1, 2, C2), (0, 64, 0, 64, 64, 1, 3, C2), (1, 384, 128, 128, 64, 3, 2, C2), (1, 576, 192, 320, 64, 3, 2, C2),
         (1, 768, 256, 512, 64, 5, 2, C2), (1, 1088, 320, 832, 64, 5, 2, C2)]

# id, in_dim, out_dim, segments (kind, in_off, gate_off, out_off, mul, dim, act, cst), 16-byte form forward?, backward?
GATE_CASES = [
    ("config_energy_layer", 1408, 1152, LAYER, 1, 1),
    ("segments_out_of_row_order", 1408, 1152, LAYER[::-1], 1, 1),
    ("six_channels", 66, 54, [(0, 0, 0, 0, 6, 1, 2, C2), (1, 18, 6, 6, 6, 3, 2, C2), (1, 36, 12, 24, 6, 5, 2, C2)], 0, 0),
    ("input_offset_off_16_bytes", 50, 32, [(0, 0, 0, 0, 8, 1, 2, C2), (1, 26, 8, 8, 8, 3, 2, C2)], 0, 0),
    ("row_width_off_16_bytes", 42, 32, [(0, 0, 0, 0, 8, 1, 2, C2), (1, 16, 8, 8, 8, 3, 2, C2)], 0, 0),
    ("input_columns_nobody_reads", 48, 32, [(0, 0, 0, 0, 8, 1, 2, C2), (1, 24, 16, 8, 8, 3, 2, C2)], 1, 0),
    ("output_columns_nobody_writes", 40, 36, [(0, 0, 0, 0, 8, 1, 2, C2), (1, 16, 8, 12, 8, 3, 2, C2)], 0, 1),
    ("overlapping_input_blocks", 40, 32, [(0, 0, 0, 0, 8, 1, 2, C2), (0, 4, 0, 8, 4, 1, 2, C2), (1, 16, 8, 8, 8, 3, 2, C2)], 0, 0),
    ("gated_block_past_the_row", 36, 32, [(0, 0, 0, 0, 8, 1, 2, C2), (1, 16, 8, 8, 8, 3, 2, C2)], 0, 0),
    ("dim_7", 68, 60, [(0, 0, 0, 0, 4, 1, 2, C2), (1, 12, 4, 4, 8, 7, 2, C2)], 1, 1),
    ("dim_9", 44, 40, [(0, 0, 0, 0, 4, 1, 2, C2), (1, 8, 4, 4, 4, 9, 2, C2)], 0, 0),
    ("scalar_block_with_dim_3", 24, 24, [(0, 0, 0, 0, 8, 3, 2, C2)], 0, 0),
]


@pytest.mark.parametrize("case", GATE_CASES, ids=[c[0] for c in GATE_CASES])
def test_gate_kernel_choice(case):
    from e3_layers_amd.backend import lib as L

    _, in_dim, out_dim, segs, fwd, bwd = case
    arr = (L.GateSeg * len(segs))()
    for i, s in enumerate(segs):
        (arr[i].kind, arr[i].in_off, arr[i].gate_off, arr[i].out_off, arr[i].mul, arr[i].dim, arr[i].act, arr[i].cst) = s
    lib = L.load()
    assert lib.e3k_gate_path(in_dim, out_dim, arr, len(segs), 0) == fwd
    assert lib.e3k_gate_path(in_dim, out_dim, arr, len(segs), 1) == bwd


def test_gate_path_refuses_bad_tables():
    from e3_layers_amd.backend import lib as L

    arr = (L.GateSeg * 1)()
    (arr[0].kind, arr[0].in_off, arr[0].gate_off, arr[0].out_off, arr[0].mul, arr[0].dim, arr[0].act, arr[0].cst) = (0, 0, 0, 0, 0, 1, 2, C2)
    lib = L.load()
    assert lib.e3k_gate_path(8, 8, arr, 1, 0) == -1      # mul 0
    arr[0].mul = 8
    assert lib.e3k_gate_path(8, 8, arr, 0, 0) == -1      # no segments
    assert lib.e3k_gate_path(0, 8, arr, 1, 0) == -1
    assert lib.e3k_gate_path(8, 8, arr, 1, 0) == 1


@pytest.mark.parametrize("rows,nets,tile", [
    (1, 1, 16), (64, 1, 16), (513, 5, 16),      # the knot rows of config_energy's radial tables: 9 tiles of 64 x 5 nets
    (16320, 1, 16), (16321, 1, 64),             # 255 and 256 tiles of 64 rows
    (3264, 5, 16), (3265, 5, 64),               # 51 x 5 = 255, 52 x 5 = 260
    (70656, 1, 64), (70656, 5, 64),             # per-edge rows
])
def test_mlp_row_tile(rows, nets, tile):
    from e3_layers_amd.backend import lib as L

    assert L.load().e3k_mlp_tile_rows(rows, nets) == tile


def test_mlp_row_tile_refuses_bad_counts():
    from e3_layers_amd.backend import lib as L

    lib = L.load()
    assert lib.e3k_mlp_tile_rows(-1, 1) == -1
    assert lib.e3k_mlp_tile_rows(10, 0) == -1
    assert lib.e3k_mlp_tile_rows(10, 9) == -1
