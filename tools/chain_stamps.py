"""Per-job clock stamps of the serial chain that ends the optimisation step (hb_debug_set("chain_stamps", 1)): thread 0 of
the chain kernel keeps a stamp of the kernel entry, of the end of its load phase and of the end of every job, and stores
them when the kernel ends.  Printed for the plain (chain_hoist=0) and the hoisted form of the same plan.

    python tools/chain_stamps.py cfg2
"""
import ctypes
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import henbun_amd as hb  # noqa: E402
from henbun_amd import _lib, hip_ops as H  # noqa: E402
import bench  # noqa: E402

name = sys.argv[1] if len(sys.argv) > 1 else "cfg2"
cfg = bench.CONFIGS[name]
buf = (ctypes.c_ulonglong * 16)()
_lib.lib().call("hb_chain_stamps", buf, 16)      # allocates the device buffer before any stream capture
for hoist in (0, 1):
    H.debug_set("chain_stamps", 1)
    H.debug_set("chain_hoist", hoist)
    with hb.settings.temp_settings(hb.settings.get_settings()):
        m, dp_reduce, _ = bench.build_model(name, cfg, 1, 0, "float32", cfg["n"])
        opt = m.ELBO()
        opt.compile(dp_reduce=dp_reduce)
        opt.optimize(maxiter=5, minibatch_size=cfg["n"])
        plan = opt.last_plan
    H.debug_clear()
    rows = []
    for _ in range(20):
        opt._run_steps(plan, 1)
        torch.cuda.synchronize()
        _lib.lib().call("hb_chain_stamps", buf, 16)
        k = int(buf[0])
        rows.append(np.diff(np.array([buf[i] for i in range(1, k + 1)], dtype=np.int64)))
    med = np.median(np.array(rows), axis=0)
    print("%s chain_hoist=%d  cycles (median of 20 steps): load phase %d | jobs %s | total %d"
          % (name, hoist, med[0], " ".join("%d" % c for c in med[1:]), med.sum()))
