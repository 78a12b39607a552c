"""The host side of the raw-BVH path (no GPU): read_bvh_raw + the host numerics == read_bvh, topology grouping, which files
the device path takes, the GMR_DATASET_BVH switch, and the pipeline with raw clips."""
import os

import numpy as np
import pytest

import bvh_synth
from conftest import GOLDEN

BVH = os.path.join(GOLDEN, "synthetic.bvh")


def test_raw_plus_host_numerics_is_read_bvh():
    from general_motion_retargeting_amd.utils import lafan1
    raw = lafan1.read_bvh_raw(BVH)
    assert raw.channels == 3 and raw.order == "zyx" and len(raw) == 12 and raw.rows.shape == (12, 3 + 3 * 22)
    assert raw.rows.dtype == np.float64 and raw.offsets.shape == (22, 3) and raw.frametime > 0
    a, b = lafan1.bvh_from_raw(raw), lafan1.read_bvh(BVH)
    assert a.bones == b.bones and a.order == b.order and a.frametime == b.frametime
    for k in ("parents", "offsets", "pos", "eulers", "quats"):
        assert np.array_equal(getattr(a, k), getattr(b, k)), k
    g = np.load(os.path.join(GOLDEN, "g_bvh.npz"))
    names = [str(x) for x in g["names"]]
    assert np.abs(lafan1.packed_from_raw(raw, names) - g["poses"]).max() <= 1e-14
    assert np.array_equal(lafan1.packed_from_raw(raw, names[:5]), lafan1.load_lafan1_packed(BVH, names[:5])[0])
    hdr = lafan1.read_bvh_raw(BVH, header_only=True)
    assert len(hdr) == 0 and hdr.names == raw.names and hdr.channels == 3
    # np.radians is one multiply by the double pi / 180: what the kernel does
    x = np.random.default_rng(0).uniform(-720, 720, 10000)
    assert np.array_equal(np.radians(x), x * (np.pi / 180.0))


def test_written_file_round_trips(tmp_path):
    from general_motion_retargeting_amd.utils import lafan1
    r = bvh_synth.make_raw(9, seed=5)
    f = str(tmp_path / "x.bvh")
    bvh_synth.write_bvh(f, r.names, r.parents, r.offsets, r.rows)
    back = lafan1.read_bvh_raw(f)
    assert lafan1.topology_key(back) == lafan1.topology_key(r)
    assert np.array_equal(back.rows, r.rows) and np.array_equal(back.offsets, r.offsets)


def test_topology_key_and_selection():
    from general_motion_retargeting_amd.utils import lafan1
    a, b = bvh_synth.make_raw(3, seed=1), bvh_synth.make_raw(8, seed=2, offset_scale=1.3)
    assert lafan1.topology_key(a) == lafan1.topology_key(b)                     # bone lengths are per-clip data
    c = bvh_synth.make_raw(3, seed=1, order="xyz")
    d = lafan1.BvhRaw(a.names + ["Extra"], np.append(a.parents, 3), np.vstack([a.offsets, [[0, 1, 0]]]), 3, "zyx", a.frametime,
                      np.hstack([a.rows, np.zeros((3, 3))]))
    assert len({lafan1.topology_key(x) for x in (a, c, d)}) == 3
    sp, sr = lafan1.selection(a.names, ["Hips", "LeftFootMod", "RightFootMod", "Head"])
    n = a.names.index
    assert sp == [n("Hips"), n("LeftFoot"), n("RightFoot"), n("Head")] and sr == [n("Hips"), n("LeftToe"), n("RightToe"), n("Head")]
    with pytest.raises(ValueError):
        lafan1.selection(a.names, ["NoSuchBone"])


def test_which_files_the_device_path_takes():
    from general_motion_retargeting_amd.utils import lafan1
    a = bvh_synth.make_raw(4)
    assert lafan1.device_takes(a) and lafan1.device_takes(bvh_synth.make_raw(4, channels=6, order="yxz"))
    J = len(a.parents)
    nine = lafan1.BvhRaw(a.names, a.parents, a.offsets, 9, "zyx", a.frametime, np.ones((4, 3 + 9 * (J - 1))))
    assert not lafan1.device_takes(nine)
    assert lafan1.packed_from_raw(nine, ["Hips", "LeftFootMod"]).shape == (4, 2, 7)      # ... the host functions do
    assert not lafan1.device_takes(lafan1.BvhRaw(a.names, a.parents, a.offsets, 3, None, a.frametime, a.rows))
    assert not lafan1.device_takes(lafan1.BvhRaw(a.names, a.parents, a.offsets, 3, "zyz", a.frametime, a.rows))
    assert not lafan1.device_takes(lafan1.BvhRaw(a.names, a.parents, a.offsets, 3, "zyx", a.frametime, a.rows[:, :-1]))


def test_bvh_path_selection(monkeypatch):
    from general_motion_retargeting_amd import dataset
    monkeypatch.setattr(dataset, "post_path", lambda: "device")
    monkeypatch.delenv("GMR_DATASET_BVH", raising=False)
    assert dataset.bvh_path() == "device"
    monkeypatch.setenv("GMR_DATASET_BVH", "host")
    assert dataset.bvh_path() == "host"
    monkeypatch.setenv("GMR_DATASET_BVH", "device")
    monkeypatch.setattr(dataset, "post_path", lambda: "host")                   # no GPU / GMR_DATASET_POST=host
    assert dataset.bvh_path() == "host"


def test_loader_returns_the_raw_parse_only_when_asked(tmp_path):
    from general_motion_retargeting_amd import dataset
    from general_motion_retargeting_amd.utils import lafan1
    names = ["Hips", "LeftFootMod"]
    raw = dataset._load_bvh_clip((BVH, names, True))
    assert isinstance(raw, lafan1.BvhRaw) and len(raw) == 12
    packed = dataset._load_bvh_clip((BVH, names, False))
    assert np.array_equal(packed, dataset._load_bvh_clip((BVH, names))) and packed.shape == (12, 2, 7)
    assert np.array_equal(dataset._BvhLoad(names)(BVH), packed) and isinstance(dataset._BvhLoad(names, True)(BVH), lafan1.BvhRaw)
    with pytest.raises(ValueError):
        dataset._load_bvh_clip((BVH, ["NoSuchBone"], True))


def test_pipeline_with_injected_raw_clips(tmp_path, capsys):
    """DatasetPipeline hands raw clips to a staged retargeter as they arrive; a file that fails to parse is printed and skipped."""
    from general_motion_retargeting_amd import dataset
    from general_motion_retargeting_amd.utils import lafan1
    clips = {f"c{i}": bvh_synth.make_raw(n, seed=i) for i, n in enumerate((9, 4, 0, 7))}

    def load(src):
        if src == "bad":
            raise ValueError("ragged motion block")
        return clips[src]

    class Staged:
        def __init__(self):
            self.batches, self.cur = [], None

        def begin(self, longest, max_clips, budget):
            self.cur = {"T": longest, "cap": min(max_clips, budget // max(longest, 1)), "clips": []}

        def add(self, clip):
            assert isinstance(clip, lafan1.BvhRaw)
            if len(self.cur["clips"]) >= self.cur["cap"] or len(clip) > self.cur["T"]:
                return False
            self.cur["clips"].append(clip)
            return True

        def finish(self, files):
            self.batches.append(self.cur["clips"])
            return [{k: np.full(1, len(c)) for k in dataset.BVH_KEYS} for c in self.cur["clips"]]

    st = Staged()
    pipe = dataset.DatasetPipeline(load, st, len, dataset.BVH_KEYS, frames_budget=18, verbose=False)
    jobs = [(s, str(tmp_path / f"{s}.pkl")) for s in ("c0", "bad", "c3", "c1", "c2")]
    assert pipe.run(jobs) == 4 and pipe.stats["load_errors"] == 1 and pipe.stats["frames"] == 20
    assert "Error loading bad" in capsys.readouterr().out
    assert [len(b) for b in st.batches] == [2, 2]
    assert not os.path.exists(str(tmp_path / "bad.pkl")) and os.path.exists(str(tmp_path / "c2.pkl"))
