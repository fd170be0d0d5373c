"""Lab builds of libcp25.so whose attn_wide.hip is compiled with one of attn_fwd_wq's isolation switches, for same-box
A/B runs against the product library (tools/bench_attn.py --ab-libs, tools/ab_self_form.py --lib); every other unit is
the in-tree object, and the source is the product file, so a lab build cannot drift from the kernel it is compared with.

  python tools/lab/build_wq_lab.py parent            # -DCP25_WQ_PARENT_LOOP: round 13's loop (64 keys per iteration)
  python tools/lab/build_wq_lab.py pad               # round 17's loop: 288-B rows, 18 pieces a tile, descriptors at the head
  python tools/lab/build_wq_lab.py image             # the 16-piece image alone (-DCP25_WQ_HEAD_RSRC)
  python tools/lab/build_wq_lab.py image_gaps        # the product's flags: and the tile descriptors made in the last gaps
  python tools/lab/build_wq_lab.py <name> -DX ...    # any other combination
Writes tools/lab/libcp25_wq_<name>.so (never libcp25.so).
"""
import glob
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
CSRC = os.path.join(ROOT, "cosmos-predict2.5_amd", "csrc")
OBJ = os.path.join(ROOT, "cosmos-predict2.5_amd", "cosmos_predict2", "_lib", "obj")
NAMED = {"parent": ["-DCP25_WQ_PARENT_LOOP"],
         "pad": ["-DCP25_WQ_PAD_IMAGE", "-DCP25_WQ_HEAD_RSRC"],               # round 17's loop: 288-B rows, 18 pieces
         "pad_gaps": ["-DCP25_WQ_PAD_IMAGE"],                                 # + the descriptors made in gaps
         "image": ["-DCP25_WQ_HEAD_RSRC"],                                    # the 16-piece image alone
         "image_gaps": [],                                                    # the product: + the descriptors in gaps
         "k64_image": ["-DCP25_WQ_ITER_TILES=1", "-DCP25_WQ_HEAD_RSRC"],      # the 16-piece image, 64 keys per iteration
         "k64_gaps": ["-DCP25_WQ_ITER_TILES=1", "-DCP25_WQ_PAD_IMAGE"]}       # the parent + the descriptors in gaps


def main():
    name, defs = sys.argv[1], sys.argv[2:]
    defs = defs if defs or name not in NAMED else NAMED[name]
    subprocess.check_call(["make", "-s", "-C", CSRC, "-j8"])
    obj = os.path.join(OBJ, f"attn_wide_lab_{name}.o")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-O3", "-fPIC", "-std=c++17",
                           "-fhip-fp32-correctly-rounded-divide-sqrt", "-I" + os.path.join(ROOT, "include"), "-I" + CSRC,
                           "-fno-honor-nans", "-fno-slp-vectorize", *defs, "-c", os.path.join(CSRC, "attn_wide.hip"),
                           "-o", obj])
    others = [o for o in sorted(glob.glob(os.path.join(OBJ, "*.o")))
              if not os.path.basename(o).startswith("attn_wide")]
    out = os.path.join(ROOT, "tools", "lab", f"libcp25_wq_{name}.so")
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-shared", "-fPIC", "-o", out, obj, *others])
    print(out, " ".join(defs))


if __name__ == "__main__":
    main()
