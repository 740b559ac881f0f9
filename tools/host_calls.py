#!/usr/bin/env python3
"""Per-call time of the host decode entry points on code A at batch 1 and 4096, for the library FPLDPC_LIB_PATH
names or the tree's: the median of the timed calls after three warm-up calls, one JSON line.  For A/B runs start
one process per library, alternating (profiles/r19/host_core/)."""
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fixedpointldpc_amd as F  # noqa: E402

code = F.Code.array(47, 5)
snr, sigma = F.snr_sigma(4.5, code.rate)
llr = F.channel_llr(123456789, 0, 4096, code.n, snr, sigma, dtype=np.int16)
kinds = {
    "flood": (F.Decoder(code), lambda d, x: d.decode_host(x)),
    "float": (F.Decoder(code), lambda d, x: d.decode_float_host(x / 16.0, post=True)),
    "layered": (F.LayeredDecoder(code), lambda d, x: d.decode_host(x)),
    "layered_minsum": (F.LayeredDecoder(code, post_bits=12, msg_bits=10, check="minsum", scale_16=12),
                       lambda d, x: d.decode_host(x)),
    "minsum": (F.MinSumDecoder(code, scale_16=12), lambda d, x: d.decode_host(x)),
}
out = {"lib": os.environ.get("FPLDPC_LIB_PATH", "tree"), "build_id": F.lib().fpldpc_kernel_build_id().decode()}
for name, (dec, call) in kinds.items():
    for B in (1, 4096):
        x = llr[:B]
        reps = (200 if B == 1 else 20) if name != "float" else (50 if B == 1 else 5)
        for _ in range(3):
            call(dec, x)
        ts = []
        for _ in range(reps):
            t = time.perf_counter()
            call(dec, x)
            ts.append(time.perf_counter() - t)
        out[f"{name}_b{B}_us"] = round(1e6 * float(np.median(ts)), 1)
print(json.dumps(out))
