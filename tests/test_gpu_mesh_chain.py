"""GPU: the whole chain of the -m mesh in one run of the driver, -mw -> -mc -> -mh -> -mt -> -ms -> -mv: every stage takes the mesh of the
stage before it.  The driver tests of the single passes cover -mw -> X and X -> -ms; the links between -mc, -mh and -mt are only here."""
import os

import numpy as np
import pytest

import deform_mesh_cases as mc
import mesh_driver_cases as drv
from kintinuous_amd import mesh_components_ref as comp_ref

pytestmark = pytest.mark.gpu


def _result(path):
    """the numbers of a sidecar's `result` line"""
    line = [l.split() for l in open(path).read().splitlines() if l.startswith("result ")]
    assert len(line) == 1
    return [int(x) if x.isdigit() else x for x in line[0][1:]]


def test_driver_runs_the_whole_chain_on_the_crab_walk(tmp_path):
    """kintinuous_hip -m -mw -mc k -mh e -mt 5 -ms 0.15 -mv on the out-and-back crab-walk.  A reporting run (-m -mw -mc 1 -mh 0) gives the
    components of the welded mesh and the simple loops on them: k is the size of the smallest component plus one, as in
    test_driver_mc_on_the_welded_crab_walk, so that it goes and the largest stays; e is the length of the shortest loop on a component that
    stays (test_driver_mh_on_the_welded_crab_walk takes the shortest of all, which -mc k may just have dropped), so that the hole stage
    has a loop to fill.  Every stage's counts are then the counts the stage before it wrote, -mt leaves the faces alone, -ms takes the
    smoothed mesh, -mv views the last one, and the run without -mt is the same up to the filled mesh."""
    run = drv.crab_walk_driver(tmp_path)
    rd = lambda p: open(p, "rb").read()
    _, p0 = run("report", "-m", "-mw", "-mc", "1", "-mh", "0")
    mesh_files = [".comp", ".holes", ".ply", ".weld", "_comp.ply", "_weld.ply"]
    assert [e for e in drv.outputs(tmp_path, p0) if e.endswith(".ply") or e in (".weld", ".comp", ".holes", ".smooth", ".simp", ".view")] == mesh_files
    cv, ct = mc.read_ply(p0 + "_comp.ply")                                                   # the mesh .holes speaks of: its loop labels are these vertices
    labels = comp_ref.labels_of(len(cv), ct)
    sizes = np.bincount(labels[ct[:, 0]], minlength=len(cv))                                  # triangles per component, at the component's label
    present = np.sort(sizes[sizes > 0])
    assert present[0] < present[-1], "the welded crab-walk mesh has components of one size only: no threshold separates them"
    k = int(present[0]) + 1
    loops = [(int(a), int(b)) for tag, a, b, c in (l.split() for l in open(p0 + ".holes").read().splitlines() if l.startswith("loop "))]
    staying = sorted(edges for label, edges in loops if sizes[labels[label]] >= k)
    print("crab-walk: components of %s ... %s triangles, k = %d; %d simple loops, %d on components that stay, lengths %s"
          % (present[:3].tolist(), present[-2:].tolist(), k, len(loops), len(staying), staying[:8]))
    assert staying and 3 <= staying[0] <= 256, "no simple loop of at most 256 edges is left on the components that -mc %d keeps" % k
    e = staying[0]

    chain = ["-m", "-mw", "-mc", str(k), "-mh", str(e)]
    _, p1 = run("full", *chain, "-mt", "5", "-ms", "0.15", "-mv")
    _, p2 = run("unsmoothed", *chain, "-ms", "0.15", "-mv")
    views = [".view", "_simp_view_color.ppm", "_simp_view_depth.pgm", "_simp_view_model.ppm"]
    assert drv.outputs(tmp_path, p2) == sorted(drv.outputs(tmp_path, p0) + ["_fill.ply", ".simp", "_simp.ply"] + views)
    assert drv.outputs(tmp_path, p1) == sorted(drv.outputs(tmp_path, p2) + [".smooth", "_smooth.ply"])
    weld, comp, holes, smooth, simp = (_result(p1 + ext) for ext in (".weld", ".comp", ".holes", ".smooth", ".simp"))
    print("chain: weld %s, comp %s, holes %s, smooth %s, simp %s" % (weld, comp[:4], holes[:4] + holes[9:10], smooth[:2], simp[:4]))
    assert comp[0] == weld[1] and comp[2] == weld[2]                                          # .comp n_in, m_in = .weld n_out, triangles
    assert holes[0] == comp[1] and holes[2] == comp[3]                                        # .holes n_in, m_in = .comp n_out, m_out
    assert smooth[0] == holes[1] and smooth[1] == holes[3]                                    # .smooth n, m = .holes n_out, m_out
    assert simp[0] == smooth[0] and simp[2] == smooth[1]                                      # .simp n_in, m_in = .smooth n, m
    assert weld[1] != weld[0] and comp[3] < comp[2] and holes[9] >= 1                         # ... and each link says something
    filled, smoothed = mc.read_ply(p1 + "_fill.ply"), mc.read_ply(p1 + "_smooth.ply")
    assert np.array_equal(smoothed[1], filled[1]) and len(smoothed[0]) == len(filled[0]) == smooth[0]
    assert rd(p1 + "_simp.ply") != rd(p2 + "_simp.ply")                                       # -ms took the smoothed mesh
    assert open(p1 + ".view").read().splitlines()[0] == "file " + os.path.basename(p1) + "_simp.ply"
    for ext in drv.outputs(tmp_path, p2):
        if "simp" not in ext and "view" not in ext:                                           # up to and including _fill.ply and .holes
            assert rd(p1 + ext) == rd(p2 + ext), ext
    assert {"_fill.ply", ".holes", "_comp.ply", ".comp", "_weld.ply", ".weld", ".ply"} <= {x for x in drv.outputs(tmp_path, p2) if "simp" not in x and "view" not in x}
