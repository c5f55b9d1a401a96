#!/usr/bin/env python3
"""Write transplat_amd/csrc/turbo_lut.h from matplotlib's turbo table (build-time only: the
package never imports matplotlib). Usage: python tools/gen_turbo_lut.py"""
from pathlib import Path

import matplotlib

OUT = Path(__file__).resolve().parent.parent / "transplat_amd" / "csrc" / "turbo_lut.h"


def main() -> None:
    colors = matplotlib.colormaps["turbo"].colors
    assert len(colors) == 256 and all(len(c) == 3 for c in colors)
    lines = [
        "// The 256-entry turbo colour map (A. Mikhailov, Google, Apache-2.0) as listed in",
        f"// matplotlib.colormaps[\"turbo\"].colors of matplotlib {matplotlib.__version__} (_cm_listed.py): data, written by",
        "// tools/gen_turbo_lut.py. Entries are the table's decimal values; the kernel rounds them to fp32.",
        "#pragma once",
        "",
        "namespace tsplat {",
        "namespace frames {",
        "",
        "__device__ const float kTurbo[256][3] = {",
    ]
    for r, g, b in colors:
        lines.append(f"    {{{r!r}f, {g!r}f, {b!r}f}},")
    lines += ["};", "", "}  // namespace frames", "}  // namespace tsplat", ""]
    OUT.write_text("\n".join(lines))


if __name__ == "__main__":
    main()
