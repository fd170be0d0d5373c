"""CPU: attn_fwd_wq's LDS image of a 64-key K or V tile (csrc/attn_wq_image.h: 256-B rows, four to a 1-KiB DMA piece,
pieces 1056 B apart), compiled alone by the host compiler (tests/host/attn_wq_image_main.cpp prints its tables) and
checked here with a bank model written independently of the header:

* off() maps the 64 x 16 (row, 16-B chunk) slots one-to-one onto 16 pieces x 64 lanes, the image is 16 896 B, and
  every wave's four pieces land where the kernel's M0 arithmetic (base 1056 w, step 4224 j) puts them;
* lane base + immediate is the address of the row and column each lane of a fragment read wants, for the 4 key blocks
  x 4 d steps of the K reads and the 2 key steps x 2 halves x 8 column blocks of the V reads, so every immediate is
  lane-uniform;
* no bank conflict in any of those reads. The model is the LDS's documented service order: 64 banks of 4 B,
  bank = (a / 4) mod 64; a ds_read_b128 is served in four groups of 16 lanes ({0-3, 12-15, 20-27}, {4-11, 16-19,
  28-31} and the same + 32), a ds_read_b64_tr_b16 in two halves of 32 lanes; lanes of one group conflict when they
  touch a bank at different addresses. The same model finds attn_fwd_m16's 288-B rows conflict-free and plain 256-B
  rows 8-way (K) and 8-way (V) conflicted, so it can tell a good image from a bad one.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "cosmos-predict2.5_amd", "csrc")

B128_GROUPS = [[*range(0, 4), *range(12, 16), *range(20, 28)], [*range(4, 12), *range(16, 20), *range(28, 32)]]
B128_GROUPS += [[l + 32 for l in g] for g in B128_GROUPS]
TR_GROUPS = [list(range(0, 32)), list(range(32, 64))]


@pytest.fixture(scope="module")
def img(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("wqimg") / "attn_wq_image_main")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-I", CSRC,
                    os.path.join(ROOT, "tests", "host", "attn_wq_image_main.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True, check=True)
    t = {"off": {}, "slot": {}, "piece": {}, "wave": {}, "kbase": {}, "vbase": {}, "kimm": {}, "vimm": {}}
    for line in r.stdout.splitlines():
        w = line.split()
        v = [int(x) for x in w[1:] if x.lstrip("-").isdigit()]
        if w[0] == "image":
            t["image"] = dict(zip(w[0::2], [int(x) for x in w[1::2]]))
        elif w[0] == "off":
            t["off"][(v[0], v[1])] = v[2]
            t["slot"][(v[0], v[1])] = (v[3], v[4])
        elif w[0] == "piece":
            t["piece"][(v[0], v[1])] = (v[2], v[3], v[4])
        elif w[0] == "wave":
            t["wave"][(v[0], v[1])] = (v[2], v[3])
        elif w[0] == "base":
            t["kbase"][v[0]], t["vbase"][v[0]] = v[1], v[2]
        elif w[0] == "kimm":
            t["kimm"][(v[0], v[1])] = v[2]
        elif w[0] == "vimm":
            t["vimm"][(v[0], v[1], v[2])] = v[3]
    return t


def conflicts(addrs, nbytes, groups):
    """Extra LDS cycles of one wave-instruction: per lane group and bank, the distinct addresses beyond the first."""
    extra = 0
    for grp in groups:
        banks = {}
        for lane in grp:
            for b in range(addrs[lane], addrs[lane] + nbytes, 4):
                banks.setdefault((b // 4) % 64, set()).add(b)
        extra += max(len(s) for s in banks.values()) - 1
    return extra


def k_want(lane, kb, s):  # (row, byte column) lane (c16, g) of the K fragment of key block kb, d step s reads
    return 16 * kb + (lane & 15), 64 * s + 16 * (lane >> 4)


def v_want(lane, ks, hf, f):  # the same for a transposed V read of key step ks, half hf, column block f
    return 32 * ks + 16 * hf + 4 * (lane >> 4) + ((lane & 15) >> 2), 32 * f + 8 * (lane & 3)


def test_image_size_and_bijection(img):
    assert img["image"] == {"image": 16896, "pieces": 16, "piece_bytes": 1024, "rows": 64, "row_bytes": 256}
    offs = img["off"]
    assert len(offs) == 64 * 16 and len(set(offs.values())) == 1024
    assert all(o % 16 == 0 and 0 <= o and o + 16 <= 16896 for o in offs.values())
    # 16 pieces x 64 lanes, each slot exactly once, and the DMA lane that owns a slot brings that row and column
    slots = set(img["slot"].values())
    assert slots == {(p, l) for p in range(16) for l in range(64)}
    for (row, chunk), (p, lane) in img["slot"].items():
        prow, pcol, dst = img["piece"][(p, lane)]
        assert (prow, pcol) == (row, 16 * chunk) and dst == offs[(row, chunk)] == 1056 * p + 16 * lane
    # a piece is 1024 contiguous bytes inside the image; pieces do not overlap
    for p in range(16):
        dsts = sorted(img["piece"][(p, l)][2] for l in range(64))
        assert dsts == list(range(1056 * p, 1056 * p + 1024, 16)) and dsts[-1] + 16 <= 16896
    # a piece's four rows: r, r + 8, r + 16, r + 24 of one 32-row group, 16 lanes each
    for p in range(16):
        rows = [img["piece"][(p, l)][0] for l in range(64)]
        r0 = 32 * (p >> 3) + (p & 7)
        assert rows == [r0 + 8 * (l >> 4) for l in range(64)]


def test_wave_pieces(img):
    """Wave w moves pieces w + 4 j at LDS byte 1056 w + 4224 j of the image: all 16, each once."""
    assert sorted(p for p, _ in img["wave"].values()) == list(range(16))
    for (w, j), (p, dst) in img["wave"].items():
        assert p == w + 4 * j and dst == 1056 * w + 4224 * j == img["piece"][(p, 0)][2]


def test_k_reads_lane_uniform_and_conflict_free(img):
    for kb in range(4):
        for s in range(4):
            addrs = [img["kbase"][l] + img["kimm"][(kb, s)] for l in range(64)]
            for l in range(64):
                row, col = k_want(l, kb, s)
                assert addrs[l] == img["off"][(row, col // 16)], (kb, s, l)
            assert conflicts(addrs, 16, B128_GROUPS) == 0, (kb, s)
    assert max(img["kimm"].values()) + 16896 < 65536  # the ds_read offset field, second image included


def test_v_reads_lane_uniform_and_conflict_free(img):
    for ks in range(2):
        for hf in range(2):
            for f in range(8):
                addrs = [img["vbase"][l] + img["vimm"][(ks, hf, f)] for l in range(64)]
                for l in range(64):
                    row, col = v_want(l, ks, hf, f)
                    assert addrs[l] == img["off"][(row, col // 16)] + col % 16, (ks, hf, f, l)
                assert conflicts(addrs, 8, TR_GROUPS) == 0, (ks, hf, f)
    assert max(img["vimm"].values()) + 16896 < 65536


@pytest.mark.parametrize("stride, want", [(288, 0), (256, 7)])
def test_bank_model_tells_images_apart(stride, want):
    """The model on row-major images: attn_fwd_m16's 288-B rows are conflict-free, plain 256-B rows put the 8 rows of a
    lane group on one bank window (7 extra cycles per group: 8-way)."""
    k = [k_want(l, 1, 2) for l in range(64)]
    v = [v_want(l, 1, 0, 3) for l in range(64)]
    assert conflicts([r * stride + c for r, c in k], 16, B128_GROUPS) == want * 4
    assert conflicts([r * stride + c for r, c in v], 8, TR_GROUPS) == want * 2
