"""CPU: the grid rule the mask families share (csrc/vr_mask_host.h) under AddressSanitizer + UBSan in
a stand-alone program, tools/host_sanitize/mask_harness.cpp: every reason code at its boundary, a
refused grid left untouched, and per family the text each reason code maps to -- compared here with
the literal strings the three family headers held while each stated the rule itself.  No GPU."""
import pytest

from harness import run_sanitized

# MaskReason 1..4: the extent, the voxel count, elem_bytes, the alignment
TEXTS = {
    "morph": ["morph extent must lie in [1, 32768]", "morph grid holds more than 2^32 - 1 voxels",
              "morph elem_bytes must be 1 or 4", "a 4-byte mask must be 4-byte aligned"],
    "maskcc": ["mask extent must lie in [1, 32768]", "mask grid holds more than 2^32 - 1 voxels",
               "mask elem_bytes must be 1 or 4", "a 4-byte mask must be 4-byte aligned"],
    "mstat": ["grid extent must lie in [1, 32768]", "grid holds more than 2^32 - 1 voxels", "elem_bytes must be 1 or 4",
              "a 4-byte array must be 4-byte aligned"],
}
# what each family's own check answers an output on its input (-22), then one element short (-28)
SMALLER = "the output buffer is smaller than the grid (see the info's voxels)"
REFUSALS = [
    ("edt", -22, "the output overlaps the mask"), ("morph", -22, "the output overlaps the mask"),
    ("label", -22, "the label buffer overlaps the mask"), ("label_records", -22, "the record buffer overlaps the mask"),
    ("select", -22, "the output overlaps the mask"), ("label_stats", -22, "the region buffer overlaps the table"),
    ("window", -22, "the output overlaps the mask"),
    ("edt", -28, SMALLER), ("morph", -28, SMALLER),
    ("label", -28, "the label buffer is smaller than the grid (see the info's voxels)"), ("label_records", 0, ""),
    ("select", -28, SMALLER), ("label_stats", -28, "the region buffer is smaller than the table (see the info's regions)"),
    ("window", -28, SMALLER), ("label_stats_labels", -22, "the region buffer overlaps the labels"),
]


@pytest.fixture(scope="module")
def harness_output(tmp_path_factory):
    return run_sanitized(tmp_path_factory.mktemp("mask"), "mask").splitlines()


def test_the_grid_rule_at_its_boundaries(harness_output):
    """The rule restated: every extent in [1, 32768] (reason 1), at most 2^32 - 1 voxels (reason 2)."""
    seen = {}
    for line in harness_output:
        w = line.replace(":", " ").split()
        if w[0] != "grid":
            continue
        ext = tuple(int(x) for x in w[1:4])
        n = ext[0] * ext[1] * ext[2]
        want = 1 if not all(1 <= e <= 32768 for e in ext) else 2 if n > 2 ** 32 - 1 else 0
        assert int(w[4]) == want and int(w[5]) == (0 if want else n), line
        seen[ext] = want
    for axis in range(3):  # 0, 1, 32768 and 32769 on each axis
        for e, want in ((0, 1), (1, 0), (32768, 0), (32769, 1)):
            ext = tuple(e if a == axis else 1 for a in range(3))
            assert seen[ext] == want, ext
    assert seen[(32768, 32768, 3)] == 0 and seen[(32768, 32768, 4)] == 2
    assert seen[(2048, 2048, 1023)] == 0 and seen[(2048, 2048, 1024)] == 2


def test_every_family_keeps_its_texts(harness_output):
    got = {}
    for line in harness_output:
        if line.startswith("text "):
            _, family, why, text = line.split(" ", 3)
            got.setdefault(family, {})[int(why)] = text
    assert got == {family: dict(enumerate(texts, 1)) for family, texts in TEXTS.items()}
    refusals = [tuple(line.split(" ", 3)[1:]) for line in harness_output if line.startswith("refusal ")]
    assert refusals == [(call, str(rc), text) for call, rc, text in REFUSALS]
