"""K3h's job lists (csrc/bwd_jobs.h), checked on the host by host/test_k3h_jobs.cpp: no device."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_k3h_job_lists_host_logic():
    """at (76, 38): every needed column of f_xx (j >= c), f_ux and f_uu (j >= c) rides in exactly one run of one unit and nothing
    else does; a unit has at most 76 columns in at most 4 runs; the full units fill at least 95 % of their slots (87 units); the
    column jobs pass the same checker with 133 units"""
    host = os.path.join(ROOT, "host")
    subprocess.check_call(["make", "-s", "-C", host, "test_k3h_jobs"])
    out = subprocess.run([os.path.join(host, "test_k3h_jobs")], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "87 units" in out.stdout and "133 units" in out.stdout, out.stdout
