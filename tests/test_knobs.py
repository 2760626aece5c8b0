"""Every MK_* knob a test sets is one the product still reads.

A test that sets a name no source reads any more runs the default again under
another label (MK_JIT_TS_DYN did: its "dyn" and "snake" variants were reruns).
"""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# a literal name handed to setenv, one assigned in os.environ, and the keys of
# the dicts that test variants hand to setenv
SETS = re.compile(r"""setenv\(\s*["'](MK_[A-Z0-9_]+)["']|environ\[\s*["'](MK_[A-Z0-9_]+)["']\s*\]\s*=[^=]|"""
                  r"""["'](MK_[A-Z0-9_]+)["']\s*:""")


def _read(paths):
    text = []
    for path in paths:
        with open(path, encoding="utf-8", errors="replace") as f:
            text.append(f.read())
    return "\n".join(text)


def test_every_knob_a_test_sets_is_read():
    tests = sorted(glob.glob(os.path.join(ROOT, "tests", "**", "*.py"), recursive=True))
    names = {n for m in SETS.finditer(_read(tests)) for n in m.groups() if n}
    assert len(names) >= 20 and "MK_JIT_TILE_SORT" in names and "MK_JIT_LOOP_UNROLL" in names, sorted(names)
    product = [p for ext in ("py", "cpp", "hip", "h", "inc")
               for p in glob.glob(os.path.join(ROOT, "misaka-net_amd", "**", "*." + ext), recursive=True)]
    source = _read(sorted(product) + [os.path.join(ROOT, "__graft_entry__.py")])
    literals = set(re.findall(r"""["'](MK_[A-Z0-9_]+)["']""", source))
    dead = sorted(names - literals)
    assert not dead, f"set by a test, read by no source: {dead}"
