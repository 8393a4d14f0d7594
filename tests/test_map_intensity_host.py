"""CPU: the intensity entries of the C ABI exist and check their arguments, the four-channel restatements (map_intensity_ref.py) agree
with the three-channel ones of map_edge_data.py in x y z, and the inputs of test_gpu_map_intensity.py have the properties those tests
rely on: leaves of every size class in every insert, and no two output rows with the same x y z."""
import numpy as np
import pytest

import map_edge_data as med
import map_intensity_ref as mir

f32 = np.float32
E_INVALID, E_UNSUPPORTED = -1, -5


def _bits(a):
    return np.ascontiguousarray(a, f32).view(np.uint32)


def test_the_two_symbols_are_exported_and_the_abi_is_unchanged(soicp):
    L = soicp.load()
    for name in ("so_icp_set_cloud_intensity", "so_icp_prefilter_intensity"):
        assert hasattr(L, name) and name in soicp.EXPORTED
    assert L.so_icp_abi_version() == 4


def test_error_codes_are_the_headers(soicp):
    import os
    import re
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "so_icp.h")).read()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define (SO_ICP_E_[A-Z]+) \((-?\d+)\)", hdr)}
    assert codes["SO_ICP_E_INVALID"] == E_INVALID and codes["SO_ICP_E_UNSUPPORTED"] == E_UNSUPPORTED, codes


def test_setter_arguments_on_a_host_only_context(soicp):
    host = soicp.LidarSlamGpu(device_id=-1, plane_res=0.2)
    assert host.set_cloud_intensity(-1) == 0
    for off in (8, 18, 0, 14):
        assert host.set_cloud_intensity(off) == E_INVALID, off
    assert host.set_cloud_intensity(16) == E_UNSUPPORTED
    assert b"host-only" in host.L.so_icp_last_error(host.h)
    assert host.set_cloud_intensity(-1) == 0
    # the map of a host-only context is as it was: packed export, records with zeros behind x y z
    cloud = np.array([[1.0, 2.0, 3.0], [4.0, 5.0, 6.0]], f32)
    host.add_surf_point_cloud(cloud)
    rec = host.export_map_records(32)
    assert len(rec) == 2 and not rec[:, 12:].any()
    host.close()


@pytest.mark.parametrize("name", ["cube_faces_0.2", "leaf_faces_0.4", "rounds_0.2_33", "degenerate"])
def test_xyz_of_the_restatements_is_map_edge_datas(name):
    fam = med.family(name)
    a, b = med.PlainMap(fam.plane_res), mir.PlainMapI(fam.plane_res)
    for step, cloud in enumerate(fam.clouds):
        assert a.add(cloud) == b.add(mir.with_intensity_column(cloud, step))
        ea, eb = a.export(), b.export()
        assert ea.shape[0] == eb.shape[0] and np.array_equal(_bits(ea), _bits(eb[:, :3])), (name, step)


@pytest.mark.parametrize("name", ["pass_through", "leaves_of_64", "leaf_faces_0.2"])
def test_xyz_of_the_voxel_grid_is_map_edge_datas(name):
    pc = med.prefilter_cloud(name)
    want = med.voxel_grid(pc.cloud, pc.plane_res)
    got = mir.voxel_grid_xyzi(mir.with_intensity_column(pc.cloud, 5), pc.plane_res)
    assert np.array_equal(_bits(want), _bits(got[:, :3]))
    if name == "pass_through":
        assert np.array_equal(_bits(got), _bits(mir.with_intensity_column(pc.cloud, 5))), "the intensities pass through in input order"


def test_hand_checked_leaves():
    lone = np.array([[0.11, 0.12, 0.13, 201.5]], f32)
    assert np.array_equal(_bits(mir.voxel_grid_xyzi(lone, 0.2)), _bits(lone)), "a lone point keeps its intensity bit for bit"
    three = np.array([[0.11, 0.12, 0.13, 0.1], [0.12, 0.13, 0.11, 0.2], [0.13, 0.11, 0.12, 0.3]], f32)
    out = mir.voxel_grid_xyzi(three, 0.2)
    assert out.shape == (1, 4)
    # 0 + 0.1f = 0x3DCCCCCD, + 0.2f = 0x3E99999A (0.3f), + 0.3f = 0x3F19999A (0.6f), / 3.0f = 0x3E4CCCCD (0.2f)
    assert int(_bits(f32(0.1) + f32(0.2))[0]) == 0x3E99999A and int(_bits(f32(f32(0.1) + f32(0.2)) + f32(0.3))[0]) == 0x3F19999A
    assert int(_bits(out[0, 3])[0]) == 0x3E4CCCCD
    # the order matters: the same members summed from the other end give other bits for at least one of these triples
    rng = np.random.default_rng(0)
    differs = 0
    for _ in range(50):
        m = np.c_[rng.uniform(0.01, 0.19, (3, 3)), rng.uniform(0, 255, 3)].astype(f32)
        differs += _bits(mir.voxel_grid_xyzi(m, 0.2)[0, 3]) != _bits(mir.voxel_grid_xyzi(m[::-1], 0.2)[0, 3])
    assert differs > 0
    # a leaf joined in a later insert: the old centroid is the first member
    pm = mir.PlainMapI(0.2)
    pm.add(three)
    pm.add(np.array([[0.15, 0.15, 0.15, 100.0]], f32))
    assert pm.size() == 1 and _bits(pm.export()[0, 3]) == _bits((out[0, 3] + f32(100.0)) / f32(2.0))


def _expected_sizes(inp, step):
    """member counts of the input's leaves at insert `step`, from the way the input was built: the new points of the site and, when
    the site has been there before, its old centroid"""
    sizes = []
    first_seen = {}
    for s in range(step + 1):
        for k in np.unique(inp.site_of[s]):
            first_seen.setdefault(int(k), s)
    for k, first in first_seen.items():
        new = int((inp.site_of[step] == k).sum())
        sizes.append(new + (1 if first < step else 0))
    return sizes


@pytest.mark.parametrize("name", ["classes", "overflow", "non_finite"])
def test_every_insert_holds_leaves_of_every_size_class(name):
    inp = mir.get_input(name)
    exports, hists = mir.reference(name)
    for step in range(3):
        want = mir.class_histogram(_expected_sizes(inp, step))
        assert hists[step] == want, (name, step, hists[step], want)
        assert max(len(c) for c in inp.clouds) <= 25000
    # the sizes on both sides of every limit are there, old member included (second insert: every leaf of set A has one)
    sizes1 = sorted(set(_expected_sizes(inp, 1)))
    for s in mir.LEAF_SIZES:
        assert s in sizes1, (name, s)
    overflowing = [h[5] for h in hists]
    assert overflowing == ([1, 1, 0] if name == "overflow" else [0, 0, 0]), overflowing
    assert all(all(h[k] > 0 for k in range(5)) for h in hists), hists


def test_the_other_inputs_reach_what_they_are_for():
    exports, hists = mir.reference("cubes_33")
    inp = mir.get_input("cubes_33")
    cubes = {med.cube_of_point(p[:3]) for p in inp.clouds[0]}
    assert len(cubes) == 33 and None not in cubes, "two rounds at planeRes 0.2"
    assert all(h[0] > 0 and h[1] > 0 for h in hists), hists
    exports, hists = mir.reference("retable")
    inp = mir.get_input("retable")
    assert inp.plane_res == [0.2, 0.4, 0.4]
    # the second insert re-filters the cube on the coarser grid: leaves with several OLD members
    old = exports[0]
    per_leaf = np.unique(med.leaf_index(old[:, :3], 0.4), axis=0, return_counts=True)[1]
    assert (per_leaf >= 2).sum() > 100 and len(exports[1]) < len(exports[0]) + len(inp.clouds[1])


@pytest.mark.parametrize("name", list(mir.INPUTS))
def test_no_two_output_rows_share_xyz(name):
    exports, _ = mir.reference(name)
    for step, e in enumerate(exports):
        assert mir.distinct_xyz(e), (name, step)
    if name != "non_finite":
        assert all(np.isfinite(e).all() for e in exports)
    else:
        inp = mir.get_input(name)
        bad = ~np.isfinite(exports[-1][:, 3])
        assert bad.sum() == len(inp.poisoned) == 4 and np.isfinite(exports[-1][:, :3]).all()


@pytest.mark.parametrize("name", ["pass_through", "leaves_of_64", "long_leaves"])
def test_prefilter_outputs_have_distinct_xyz_and_the_leaves_they_are_named_for(name):
    pc = med.prefilter_cloud(name)
    sizes = []
    out = mir.voxel_grid_xyzi(mir.with_intensity_column(pc.cloud, 7), pc.plane_res, sizes)
    assert mir.distinct_xyz(out)
    if name == "leaves_of_64":
        assert {63, 64, 65, 66} <= set(sizes)
    if name == "long_leaves":
        assert sum(1 for s in sizes if s > 64) > 4096
    if name == "pass_through":
        assert len(out) == len(pc.cloud)
