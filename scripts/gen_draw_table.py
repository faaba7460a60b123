"""Writes pytorch-openpose_amd/csrc/draw_table.h: cos / sin of the integer degrees 0..359 as
hexadecimal float64 literals.  Run once; the header is the single source of truth afterwards (the
tests parse its literals and never recompute them).

Entry k is (math.cos(math.radians(k)), math.sin(math.radians(k))) as the host's libm rounds them,
except the four axis entries, which are exactly 0 and +-1 so that axis-aligned limbs are exact.
"""
import math
import os

OUT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "pytorch-openpose_amd", "csrc", "draw_table.h")

AXES = {0: (1.0, 0.0), 90: (0.0, 1.0), 180: (-1.0, 0.0), 270: (0.0, -1.0)}


def entry(k):
    return AXES.get(k) or (math.cos(math.radians(k)), math.sin(math.radians(k)))


def main():
    lines = ["// draw_table.h -- (cos, sin) of the integer degrees 0 .. 359 as float64 bits: the limb",
             "// rule of draw.hip and its statement in tests/draw_cases.py both read these literals, so no",
             "// libm decides a pixel.  Written by scripts/gen_draw_table.py; the entries at 0 / 90 / 180 /",
             "// 270 are exactly 0 and +-1.",
             "#pragma once",
             "",
             "#define OPOSE_DRAW_TABLE \\"]
    for k in range(360):
        c, s = entry(k)
        lines.append("    {%s, %s},%s" % (float(c).hex(), float(s).hex(), " \\" if k < 359 else ""))
    with open(OUT, "w") as f:
        f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
