"""The light sample whose latitude lies under the surface, and the chain's last launch.

shade_path leaves the rest of the probe's column search out when the arc of the sampled row's latitude circle that the guide's cell spans (or the
whole circle) is below the hit's tangent plane and the material's pdf for such a direction is not positive (pt_below_horizon_arc,
include/pt_detmath.h), and it does not compute or store the next bounce of a path
that the chain's last launch — or the fused loop at the depth cutoff — would queue without anybody tracing it.  Neither may change a bit: every
case here renders a small frame and compares all five buffers with the CPU checker, which knows nothing of either, and the device-counted totals
(radiance rays, shadow rays, shaded hits) between the launch chain and the fused loop, whose count of the paths that "would continue" is code of
its own, and with the counts the commit before this change left for the same cases (tests/golden/horizon_counts.json, a recording: see
tests/golden/make_horizon_counts.py).

Scene: an up-facing ground quad, a second one with reversed winding (the same normal after faceforward, through a sign flip), a quad tilted by
30 degrees and a vertical wall.  Probes: the sky gradient, and a 64 x 32 probe whose ground half is the brighter one (32 rows: no LDS copy of the
marginals, plain binary search); both must put at least 20 % of their marginal mass into rows below the horizon of an up-facing surface, so that
the skip cannot pass unexercised."""
import math

import numpy as np
import pytest

from horizon_cases import DEPTH, DEPTH_CASES, MARGIN, MATERIALS, PROBES, case_key, checker, golden_counts, quad_scene, render, run_case, same_as_checker

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def probes():
    out = {k: f().BuildCDF() for k, f in PROBES.items()}
    for name, p in out.items():  # the input condition: marginal mass in rows whose cosine is below -margin
        ct = np.cos(np.arange(p.height, dtype=np.float64) / p.height * math.pi)
        mass = float(np.asarray(p.pdfValuesY, np.float64)[ct < -MARGIN].sum())
        print(f"probe {name}: {mass:.3f} of the marginal mass below the horizon")
        assert mass >= 0.20, (name, mass)
    return out


@pytest.mark.parametrize("probe_name", list(PROBES))
@pytest.mark.parametrize("mode", [0, 1], ids=["disney", "lambert"])
@pytest.mark.parametrize("material", list(MATERIALS))
def test_every_buffer_and_count_is_what_it_was(ptlib, orc_det, monkeypatch, probes, material, mode, probe_name):
    run_case(monkeypatch, orc_det, probes, material, mode, probe_name)


@pytest.mark.parametrize("max_depth", [1, 2])
def test_the_last_launch_is_the_first_or_the_second(ptlib, orc_det, monkeypatch, probes, max_depth):
    """depth 1: the chain's only launch is its last (first and last at once); depth 2: the second launch is"""
    for material, mode, probe_name in DEPTH_CASES:
        run_case(monkeypatch, orc_det, probes, material, mode, probe_name, max_depth)


CARRIED = 0x200  # pt_stats.schedule: the last render's chains carried the sums (k_shade_carry)


@pytest.mark.parametrize("max_depth", [1, DEPTH])
@pytest.mark.parametrize("placement", ["write_back", "split", "async"])
def test_the_chain_without_carried_sums(ptlib, orc_det, monkeypatch, probes, placement, max_depth):
    """k_shade<MODE, false>: what a scene without catchers runs when the sums are not carried — the unified launch with the traversal's write-back
    (PT_CARRY_SUMS=0), and the split and asynchronous shadow placements.  Same images as the checker's, same counts as the carried chain's."""
    split = {"write_back": 0, "split": 1, "async": 2}[placement]
    for material, mode, probe_name in (("plain", 0, "sky"), ("glass", 0, "bright_ground"), ("plain", 1, "bright_ground")):
        model = quad_scene(MATERIALS[material])
        g = render(monkeypatch, model, probes[probe_name], False, mode, max_depth, split_shadow=split, carry=False)
        assert g[2]["fused_passes"] == 0 and g[2]["shade_launches"] >= 1 and not g[2]["schedule"] & CARRIED, g[2]
        same_as_checker(g, checker(orc_det, model, probes[probe_name], mode, max_depth), f"{placement}, {material}")
        carried = render(monkeypatch, model, probes[probe_name], False, mode, max_depth)
        assert carried[2]["schedule"] & CARRIED
        assert g[1] == carried[1], (g[1], carried[1])
        if max_depth == DEPTH:
            golden_counts(case_key(material, mode, probe_name, "chain"), g[1])
