"""Child process of tests/test_gpu_jitter.py: jittered renders with the
MCPT_DEBUG build of the library (MCPT_LIB_OVERRIDE=.../libmcpt_hip_debug.so).
Prints one JSON line per case with the bounds-check violation count and a
digest of the result.  Test infrastructure."""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from montecarlopathtracing_amd import _lib as L  # noqa: E402
from montecarlopathtracing_amd import render as R  # noqa: E402
from montecarlopathtracing_amd import scene as S  # noqa: E402
from tests import scenes  # noqa: E402


def main():
    rnd = R.Renderer(0)
    print(json.dumps({"version": L.lib().mcpt_version().decode()}), flush=True)
    w, h, frames, att = 48, 40, 6, 4  # tests/test_gpu_jitter.py: W, H, FRAMES, ATT
    for name, data, camj, depth in (("cbox", scenes.cbox(), scenes.CBOX_CAM, 4),
                                    ("mis", scenes.mis(), scenes.MIS_CAM, 12)):
        dsc = rnd.upload(data)
        st = rnd.new_state(w, h, R.default_seeds(w * h))
        rnd.render_frames(dsc, S.parse_camera(camj), st, depth, att, frames, jitter=True)
        s = rnd.stats()
        torch.cuda.synchronize()
        dg = hashlib.sha256()
        for a in (st.hist.cpu().numpy(), st.count.cpu().numpy(), st.seeds_np()):
            dg.update(np.ascontiguousarray(a).tobytes())
        print(json.dumps({"case": name, "violations": s["debug_violations"], "primary_cache": s["primary_cache"],
                          "digest": dg.hexdigest()}), flush=True)
        dsc.close()


if __name__ == "__main__":
    main()
