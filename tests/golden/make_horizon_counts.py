"""make_horizon_counts.py TREE — records tests/golden/horizon_counts.json: the device-counted totals (radiance rays, shadow rays, shaded hits) of
every case of tests/test_gpu_horizon.py, rendered on an MI355X by the package found in TREE, a built checkout of the commit whose counts are to be
pinned.  The committed file was recorded from commit 25b7d8d, the last one whose shade_path ran every light sample's column search and stored
the last launch's next bounce: the test holds the kernels that skip them to the same counts.  The CPU checker cannot supply these numbers (it
has no count of shaded hits, and it traces the rays the chain proves dead: DESIGN.md, ray accounting), so they are a recording, not a
derivation; the images of the same cases ARE compared with the checker."""
import json
import os
import sys

tree = os.path.abspath(sys.argv[1])
here = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, tree)
import optixpathtracer_amd  # noqa: E402  (bound before the test module's conftest puts this checkout's root in front)
from optixpathtracer_amd import _lib  # noqa: E402

assert os.path.dirname(os.path.abspath(optixpathtracer_amd.__file__)).startswith(tree), optixpathtracer_amd.__file__
print("library:", _lib.LIB_PATH)
sys.path.insert(1, here)
import horizon_cases as T  # noqa: E402


class Env:
    def setenv(self, k, v):
        os.environ[k] = v

    def delenv(self, k):
        os.environ.pop(k, None)


probes = {k: f().BuildCDF() for k, f in T.PROBES.items()}
counts = {"_source": "recorded by tests/golden/make_horizon_counts.py from commit 25b7d8d (before the skip) on an MI355X; see that file"}
for material in T.MATERIALS:
    for mode in (0, 1):
        for probe in T.PROBES:
            counts.update(T.run_case(Env(), None, probes, material, mode, probe, check=False))
for d in (1, 2):
    for material, mode, probe in T.DEPTH_CASES:
        counts.update(T.run_case(Env(), None, probes, material, mode, probe, d, check=False))
json.dump(counts, open(T.GOLDEN, "w"), indent=0, sort_keys=True)
print(len(counts) - 1, "cases written to", T.GOLDEN)
