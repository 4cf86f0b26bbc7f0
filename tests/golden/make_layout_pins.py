#!/usr/bin/env python3
"""Records tests/golden/layout_pins.json: the host-side layout of every handle kind as the built library answers it (tests/layout_pins.py: what is
measured and for which configurations).  Run it on the commit whose layout is to be kept -- BEFORE a change that must not move an offset or a
workspace size -- and commit the file; test_layout_pins_cpu.py then holds every later build to it.  CPU only: nothing is launched.
Run:  python tests/golden/make_layout_pins.py
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
import smtc_amd  # noqa: E402,F401
import layout_pins as L  # noqa: E402

if __name__ == "__main__":
    pins = {cid: L.measure(*case) for cid, case in L.cases().items()}
    path = os.path.join(HERE, "layout_pins.json")
    with open(path, "w") as f:
        json.dump(pins, f, indent=1, sort_keys=True)
        f.write("\n")
    print(len(pins), "configurations ->", path, os.path.getsize(path), "bytes")
