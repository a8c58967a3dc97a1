"""Child process of tests/test_gpu_env.py: the open scene lit by a 7x5 map,
rendered with the MCPT_DEBUG build of the library
(MCPT_LIB_OVERRIDE=.../libmcpt_hip_debug.so), whose k_render checks the
lookup's four texel indices.  Prints one JSON line per mode with the
bounds-check violation count and a digest of the result.  Test infrastructure."""
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
from tests import env_ref  # noqa: E402


def main():
    rnd = R.Renderer(0)
    print(json.dumps({"version": L.lib().mcpt_version().decode()}), flush=True)
    w, h, frames, att = 48, 40, 6, 4  # tests/test_gpu_env.py: W, H, FRAMES, ATT
    dsc = rnd.upload(env_ref.open_scene())
    rnd.set_environment(dsc, **env_ref.lit_environments()["map"])
    for mode in (L.MODE_EXACT, L.MODE_NOPRUNE):
        st = rnd.new_state(w, h, R.default_seeds(w * h))
        rnd.render_frames(dsc, S.parse_camera(env_ref.OPEN_CAM), st, env_ref.OPEN_DEPTH, att, frames, mode=mode)
        s = rnd.stats()
        torch.cuda.synchronize()
        dg = hashlib.sha256()
        for a in (st.hist.cpu().numpy(), st.count.cpu().numpy(), st.seeds_np()):
            dg.update(np.ascontiguousarray(a).tobytes())
        print(json.dumps({"mode": mode, "violations": s["debug_violations"], "digest": dg.hexdigest()}), flush=True)
    dsc.close()


if __name__ == "__main__":
    main()
