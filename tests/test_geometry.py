"""The detector's host-side tuning model (csrc/fdf_geometry.h: pick_geometry, make_launch_plan)
tabulated on the CPU by tests/cpp/test_geometry and pinned to tests/golden/geometry_table.txt."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
N_CASES = 771
K_DIRECT_MAX_TASKS = 1024     # fdfk::kDirectMaxTasks


def _fields(line):
    """One table line -> (shape, how R came about, {name: value})."""
    inputs, geometry, plan = line.split(" : ")
    how, *geo = geometry.split()
    shape, *ins = inputs.split()
    d = dict(kv.split("=") for kv in ins + geo + plan.split())
    w, h = shape.split("x")
    return int(w), int(h), how, d


def test_geometry_table():
    """The binary's output is the committed table byte for byte (the behaviour of the model
    before it moved into its own header), has the expected number of cases, and every line
    keeps what holds by construction: R a multiple of nsub and at least nsub; the bands cover
    the frame's centre rows with none to spare; the model's own picks stay within the LDS
    budget (40000 bytes with NMS, 35000 without); a direct launch is one round of look-back."""
    exe = os.path.join(HERE, "cpp", "test_geometry")
    res = subprocess.run([exe], capture_output=True, timeout=60)
    assert res.returncode == 0, res.stderr.decode()
    with open(os.path.join(HERE, "golden", "geometry_table.txt"), "rb") as f:
        want = f.read()
    assert res.stdout == want
    lines = res.stdout.decode().splitlines()
    assert lines[-1] == f"geometry: {N_CASES} cases, 0 failures"
    assert len(lines) == N_CASES + 1
    hows = set()
    for line in lines[:-1]:
        w, h, how, d = _fields(line)
        hows.add(how)
        R, nsub = int(d["R"]), int(d["nsub"])
        assert R % nsub == 0 and R >= nsub, line
        if how == "model":     # not forced, and some height fits the budget
            assert int(d["lds"]) <= (40000 if int(d["nms"]) else 35000), line
        assert (how == "forced") == (int(d["forced"]) != 0), line
        bands = int(d["bands"])
        assert bands * R >= h - 6 > (bands - 1) * R, line
        if int(d["direct"]):
            assert int(d["ntasks"]) <= K_DIRECT_MAX_TASKS, line
    assert hows == {"model", "forced", "floor"}
