"""Host-only: lass_amd.arch.wino4_routed (the mirror of the C dispatch that bench.py's executed-FLOP accounting uses) against the
layer list written in DESIGN.md section 4 ("Which 3x3 convs run as F(4x4,3x3)")."""
import os
import re

from lass_amd import arch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _design_lists():
    """The two fenced lists of DESIGN.md: `wino4-routed:` (10 s clips, 1024 padded frames) and `wino-routed:` (what stays F(2x2,3x3))."""
    txt = open(os.path.join(ROOT, "DESIGN.md"), encoding="utf-8").read()
    out = {}
    for key in ("wino4-routed", "wino-routed"):
        m = re.search(r"^" + key + r":\s*(.+?)\n\s*\n", txt, re.S | re.M)
        assert m, f"DESIGN.md has no '{key}:' list"
        out[key] = set(re.findall(r"[a-z_0-9]+\.conv[12]", m.group(1)))
    return out


def test_default_layer_table_matches_design_md():
    rows = arch.conv_layer_table(arch.padded_frames(arch.frames_for(160000)))
    all3x3 = {r["name"] for r in rows if r["kind"] == "3x3"}
    routed = arch.wino4_routed(rows)
    lists = _design_lists()
    assert routed == lists["wino4-routed"]
    assert all3x3 - routed == lists["wino-routed"] == {"conv_block7a.conv1", "conv_block7a.conv2"}
    assert len(all3x3) == 26 and len(routed) == 24
    for name in ("encoder_block6.conv1", "encoder_block6.conv2", "decoder_block1.conv1", "decoder_block1.conv2"):
        assert name in routed   # the 32-frame x 16-bin level: split-K F(4x4,3x3)


def test_other_frame_counts_keep_the_16_bin_level_on_f2x2():
    """The 16-bin level tiles into 32 x 16 blocks only when its frame count is a multiple of 32 (1024 padded frames per clip)."""
    for t_pad in (160, 512, 992, 2016):
        routed = arch.wino4_routed(arch.conv_layer_table(t_pad))
        for name in ("encoder_block6.conv1", "encoder_block6.conv2", "decoder_block1.conv1", "decoder_block1.conv2"):
            assert name not in routed, (t_pad, name)
    assert "decoder_block1.conv2" in arch.wino4_routed(arch.conv_layer_table(2048))


def test_wino4_off_routes_nothing():
    assert arch.wino4_routed(arch.conv_layer_table(1024), 0) == set()


def test_min_cin_threshold_applies_to_the_block_at_the_16_bin_level():
    routed = arch.wino4_routed(arch.conv_layer_table(1024), 512)   # only decoder_block1.conv1 has 768 input channels, but
    assert "decoder_block1.conv1" not in routed                      # the block routes as a whole (its cout is 384)
    assert "decoder_block2.conv1" in routed
