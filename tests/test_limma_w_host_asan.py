"""plaidhip_limma_w_solve and plaidhip_lowess as a stand-alone program under AddressSanitizer and UBSan (`make
host-asan-limma-w`), on the decks of tests/test_limma_w_ref.py and tests/test_voom_lowess_host.py with the Python restatements'
answers: never loaded into Python, never run on a device."""
import os
import struct
import subprocess

import numpy as np

from tests.helpers import limma_w_ref as wr
from tests.helpers import voom_ref as vr
from tests.test_limma_w_ref import PS, deck, sums
from tests.test_voom_lowess_host import KINDS
from tests.test_voom_lowess_host import deck as lowess_deck

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "plaid_amd", "csrc")


def test_w_solve_stand_alone_under_asan_and_ubsan(tmp_path):
    decks = []
    for p in PS:
        for kind in ("plain", "zeros", "half", "group", "p_left", "p_plus_one"):
            if kind == "group" and p == 1:
                continue
            D, x, om, K = deck(p, kind=kind)
            des, _, (Htri, b, _, nlive, _) = sums(D, x, om, K)
            ok, g, us, _ = wr.emulate_w_solve(Htri, b, nlive, des["v"])
            q = des["v"].shape[1]
            g, us = (g, us) if ok else ([np.nan] * p, [np.nan] * q)
            decks.append(struct.pack("<iiiq", p, q, int(ok), nlive) +
                         np.concatenate([Htri, b, des["v"].ravel(order="F"), g, us]).astype("<f8").tobytes())
    assert sum(1 for d in decks if struct.unpack_from("<i", d, 8)[0] == 0) >= 8
    low = []
    for kind in KINDS:
        for f_, delta_share in ((0.5, 0.01), (0.1, 0.0)):
            x, y = lowess_deck(kind, n=80)
            delta = delta_share * (x[-1] - x[0])
            ys, anchor = vr.lowess_walk(x, y, f_, 3, delta)
            low.append(struct.pack("<qidd", len(x), 3, f_, delta) + np.concatenate([x, y, ys]).astype("<f8").tobytes() +
                       anchor.astype(np.int8).tobytes())
    path = str(tmp_path / "decks.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(decks)) + b"".join(decks) + struct.pack("<i", len(low)) + b"".join(low))
    out = subprocess.run(["make", "-C", CSRC, "host-asan-limma-w", "ARGS=" + path], capture_output=True, text=True, timeout=900)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    assert "[host-asan-limma-w] ok" in out.stdout and f"{len(decks)} decks met bit for bit" in out.stdout
    assert f"{len(low)} lowess decks met bit for bit" in out.stdout
    assert "runtime error" not in out.stderr and "AddressSanitizer" not in out.stderr
