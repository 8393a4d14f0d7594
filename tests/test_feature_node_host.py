"""CPU-side checks of the feature_extraction_node shell (adapter/feature_extraction_soicp.{h,cpp}): node_config.h reads the
feature_extraction_node parameters (through adapter/wire_selftest feature-params), and the shell refuses a configuration it does
not restate -- provide_point_time 0, a Livox sensor -- before it creates any device state (adapter/feature_driver)."""
import os
import struct
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SELFTEST = os.path.join(ROOT, "adapter", "wire_selftest")
DRIVER = os.path.join(ROOT, "adapter", "feature_driver")


def _params(tmp_path, body):
    p = tmp_path / "p.yaml"
    p.write_text("/**:\n  ros__parameters:\n" + body)
    return str(p)


def _feature_params(path):
    r = subprocess.run([SELFTEST, "feature-params", path], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    return dict(line.split("=", 1) for line in r.stdout.splitlines())


def test_feature_parameters_are_read(tmp_path):
    got = _feature_params(_params(tmp_path, '    sensor: "ouster"\n    world_frame: "map"\n    PROJECT_NAME: "/so"\n'
                                            "    feature_extraction_node:\n      scan_line: 128\n      mapping_skip_frame: 2\n"
                                            "      min_range: 0.35\n      max_range: 80.0\n      filter_point_size: 5\n      provide_point_time: 1\n"))
    assert got["scan_line"] == "128" and got["mapping_skip_frame"] == "2" and got["filter_point_size"] == "5"
    assert float(got["min_range"]) == pytest.approx(0.35) and got["provide_point_time"] == "1"
    assert (got["sensor"], got["sensor_type"], got["world_frame"], got["sensor_frame"], got["PROJECT_NAME"]) == ("ouster", "1", "map", "sensor", "/so")


def test_feature_parameter_defaults(tmp_path):
    """readParameters' declared defaults (featureExtraction.cpp:122-138) and readGlobalparam's sensor "livox" """
    got = _feature_params(_params(tmp_path, "    other: 1\n"))
    assert (got["scan_line"], got["mapping_skip_frame"], got["filter_point_size"], got["provide_point_time"]) == ("4", "1", "3", "1")
    assert float(got["min_range"]) == pytest.approx(0.2) and float(got["max_range"]) == 130.0
    assert (got["sensor"], got["sensor_type"]) == ("livox", "2")


def _refused(tmp_path, body):
    bag = tmp_path / "bag.bin"
    bag.write_bytes(struct.pack("<i", 1) + struct.pack("<7d", 0, 0, 0, 0, 0, 0, 1) + struct.pack("<i", 0))
    r = subprocess.run([DRIVER, _params(tmp_path, body), str(bag), str(tmp_path / "out.bin")], capture_output=True, text=True, timeout=60)
    assert r.returncode == 1 and not (tmp_path / "out.bin").exists()
    return r.stderr


def test_shell_refuses_provide_point_time_0(tmp_path):
    err = _refused(tmp_path, '    sensor: "velodyne"\n    feature_extraction_node:\n      provide_point_time: 0\n')
    assert "feature_extraction_node.provide_point_time" in err


def test_shell_refuses_livox_and_bad_sampling(tmp_path):
    assert "livox" in _refused(tmp_path, '    sensor: "livox"\n')
    assert "filter_point_size" in _refused(tmp_path, '    sensor: "ouster"\n    feature_extraction_node:\n      filter_point_size: 0\n')
