"""What the device post-processing path needs that can be checked without a GPU: the entry point refuses a null handle, the
pool of page-locked output blocks never hands out a block that is still viewed, and the drivers fall back to the host path."""
import ctypes as C
import gc

import numpy as np

from general_motion_retargeting_amd import _lib, dataset


def test_null_handle_is_an_argument_error():
    L = _lib.lib()
    src = (_lib.PostSrc * 1)(_lib.PostSrc(1, 1, None, None))
    rc = L.gmr_postprocess_clips_dev(None, C.cast(src, C.c_void_p), 1, 36, None, 1, 1, 3, 0.0, None, None, None, None, None, None)
    assert rc == -1 and b"null fk handle" in L.gmr_last_error()


class _Block:
    """stand-in for a page-locked allocation: ordinary memory behind the same two attributes"""
    made = []

    def __init__(self, nbytes):
        self._mem = C.create_string_buffer(int(nbytes))
        self.ptr, self.nbytes = C.c_void_p(C.addressof(self._mem)), int(nbytes)
        _Block.made.append(self)


def test_a_block_returns_to_the_pool_only_when_its_last_view_is_dropped():
    _Block.made.clear()
    pool = dataset.PinnedPool(alloc=_Block)
    buf = pool.take(1000)
    a = np.frombuffer(buf, dtype=np.float64, count=50, offset=0).reshape(10, 5)
    b = np.frombuffer(buf, dtype=np.float32, count=20, offset=400)
    row = a[3:7]                                    # what a motion dict holds: a view of a view
    a[:] = 1.5
    del buf, a
    gc.collect()
    assert pool.free_blocks == 0 and pool.blocks_allocated == 1
    other = pool.take(900)                          # the first block is still viewed: a batch gets another one
    assert pool.blocks_allocated == 2 and len(_Block.made) == 2
    np.frombuffer(other, dtype=np.uint8)[:] = 0
    assert (row == 1.5).all()                       # ... and writing it leaves the kept rows alone
    del b
    gc.collect()
    assert pool.free_blocks == 0
    del row
    gc.collect()
    assert pool.free_blocks == 1
    again = pool.take(1000)                         # the freed block serves the next batch; nothing new is allocated
    assert pool.blocks_allocated == 2 and C.addressof(again) == _Block.made[0].ptr.value
    big = pool.take(10 ** 6)                        # no free block is large enough: a new one
    assert pool.blocks_allocated == 3 and big is not None
    del other, again, big
    gc.collect()
    assert pool.free_blocks == 3


def test_the_pool_keeps_a_bounded_number_of_free_blocks():
    pool = dataset.PinnedPool(alloc=_Block, keep=2)
    bufs = [pool.take(64) for _ in range(5)]
    assert pool.blocks_allocated == 5
    del bufs
    gc.collect()
    assert pool.free_blocks == 2


def test_host_path_is_selected_by_the_switch_and_without_a_gpu(monkeypatch):
    class _Lib:
        def __init__(self, n):
            self.n = n

        def gmr_device_count(self):
            return self.n

    monkeypatch.setattr(_lib, "lib", lambda: _Lib(1))
    monkeypatch.delenv("GMR_DATASET_POST", raising=False)
    assert dataset.post_path() == "device"
    monkeypatch.setenv("GMR_DATASET_POST", "host")
    assert dataset.post_path() == "host"
    monkeypatch.setenv("GMR_DATASET_POST", "device")
    monkeypatch.setattr(_lib, "lib", lambda: _Lib(0))
    assert dataset.post_path() == "host"

    def missing():
        raise _lib.GmrHipError("not built")
    monkeypatch.setattr(_lib, "lib", missing)
    assert dataset.post_path() == "host"


def test_finish_takes_the_host_path_when_told_to(monkeypatch):
    """ClipRetargeter.finish with stand-ins for the GPU calls: with GMR_DATASET_POST=host the batch goes through
    retarget_group + postprocess_clips, never through the device path"""
    calls = []
    rt = dataset.ClipRetargeter.__new__(dataset.ClipRetargeter)

    class _Sol:
        nq, nhuman = 36, 3

    class _Gmr:
        hip_solver = _Sol()
        xml_file = "unused"

        class model:
            qpos0 = np.zeros(36)

        def _flags(self, g):
            return 0

    rt.gmr, rt.height_adjust, rt.root_origin_offset, rt.offset_to_ground = _Gmr(), True, True, False
    rt._km, rt._pin, rt._dev_post, rt.timing = object(), {}, None, {}
    monkeypatch.setattr(rt, "_buf", lambda name, shape, dtype: np.zeros(shape, dtype))
    monkeypatch.setattr(rt, "_finish_device", lambda fps, lens: calls.append("device") or [])
    monkeypatch.setattr(_lib, "retarget_group", lambda jobs, flags, slices, outs=None: calls.append("group") or outs)
    monkeypatch.setattr(dataset, "postprocess_clips", lambda q, km, fps, h, o: calls.append("host") or [{"n": len(x)} for x in q])
    monkeypatch.setattr(dataset, "post_path", lambda: "host")
    rt.begin(4, 2, 100)
    assert rt.add(np.zeros((4, 3, 7))) and rt.add(np.zeros((2, 3, 7)))
    assert rt.finish([30, 30]) == [{"n": 4}, {"n": 2}] and calls == ["group", "host"]
    monkeypatch.setattr(dataset, "post_path", lambda: "device")
    rt.begin(4, 2, 100)
    assert rt.add(np.zeros((4, 3, 7)))
    rt.finish([30])
    assert calls == ["group", "host", "device"]


NINE_JOBS = [[3, 2], [1], [2], [1, 1], [3], [2], [1], [2, 1], [2]]      # clip lengths per job: more jobs than one post-processing call takes


def test_block_plan_of_nine_jobs_on_literal_values():
    """a post-processing call takes at most 8 jobs, and every further call starts at a row that is a multiple of 4"""
    ndof, nb = 5, 7
    p = dataset.plan_block(NINE_JOBS, [None] * 9, ndof, nb)
    assert len(p.calls) == 2
    (c0, r0, seg0), (c1, r1, seg1) = p.calls
    assert (c0, r0) == (0, 0) and seg0.dtype == np.int32 and seg0.tolist() == [0, 3, 5, 6, 8, 9, 10, 13, 15, 16, 18, 19]
    assert (c1, r1) == (8, 20) and seg1.dtype == np.int32 and seg1.tolist() == [0, 2]
    assert p.spans[0] == [(0, 3), (3, 5)] and p.spans[7] == [(16, 18), (18, 19)] and p.spans[8] == [(20, 22)]
    assert [len(s) for s in p.spans] == [len(l) for l in NINE_JOBS]
    assert p.rows == 24 and p.nclip == 12
    end = 0
    for name, row_bytes, n in (("root_pos", 24, 24), ("root_rot", 32, 24), ("dof_pos", ndof * 8, 24), ("local_body_pos", nb * 12, 24),
                               ("status", 4, 12)):
        off, stride = p.arrays[name][:2]
        assert off % 256 == 0 and off >= end and stride == row_bytes, name
        assert p.at(0x10000, name, 3).value == 0x10000 + off + 3 * row_bytes
        end = off + n * row_bytes
    assert list(p.arrays) == ["root_pos", "root_rot", "dof_pos", "local_body_pos", "status"]
    assert p.total == p.arrays["status"][0] + _lib.align256(48) == p.arrays["status"][0] + 256
    # the views of a host copy of the block lie where at() says the device wrote
    buf = (C.c_char * p.total)()
    rp, rr, dp, lb, status = p.views(buf)
    assert (rp.shape, rr.shape, dp.shape, lb.shape, status.shape) == ((24, 3), (24, 4), (24, ndof), (24, nb, 3), (12,))
    assert (rp.dtype, rr.dtype, dp.dtype, lb.dtype, status.dtype) == (np.float64, np.float64, np.float64, np.float32, np.int32)
    base = C.addressof(buf)
    for name, v in (("root_pos", rp), ("root_rot", rr), ("dof_pos", dp), ("local_body_pos", lb)):
        assert v[21:].ctypes.data == p.at(base, name, 21).value, name
    C.memset(p.at(base, "status", 11), 0x01, 4)
    assert p.views(buf)[4].tolist() == [0] * 11 + [0x01010101] and status.tolist() == [0] * 12        # (the status words are a copy)


def test_block_plan_without_frames_and_with_a_permutation():
    for lens in ([], [[]], [[0, 0], [0]]):
        p = dataset.plan_block(lens, [None] * len(lens), 5, 7)
        assert p.rows == 1 and p.nclip == sum(len(l) for l in lens) and p.total == 4 * 256 + _lib.align256(4 * p.nclip)
    # a raw BVH job: device position k holds clip perm[k] of the job
    p = dataset.plan_block([[5, 1, 3], [4]], [np.array([2, 0, 1]), None], 5, 7)
    assert p.dlens[0].tolist() == [3, 5, 1] and p.spans[0] == [(0, 3), (3, 8), (8, 9)] and p.spans[1] == [(9, 13)]
    assert p.to_job_order(0, p.spans[0]) == [(3, 8), (8, 9), (0, 3)]                # the spans of clips 0, 1, 2
    assert [b - a for a, b in p.to_job_order(0, p.spans[0])] == [5, 1, 3]
    assert p.to_job_order(0, np.array([30, 50, 10])).tolist() == [50, 10, 30] and p.to_job_order(1, p.spans[1]) is p.spans[1]
    assert p.spans[0] == [(0, 3), (3, 8), (8, 9)]                                    # (left in device order)
