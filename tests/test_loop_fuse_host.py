"""adapter/tsorb_loop_fuse.hpp from C++ without a device: the gather and claim logic of fuse_scene_search / search_and_fuse_scene / match_more_all against a plain
transcription of the reference's loops over mock types (tests/cxx/loop_fuse_from_cxx.cpp), the window searches through window_best_host.  The same program runs with the
device call in tests/test_gpu_window_sets.py."""
import os
import sys
import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import loop_fuse_io as IO                                             # noqa: E402


def test_adapter_from_cxx_on_the_host(tmp_path):
    import __graft_entry__ as ge
    if not os.path.exists(os.path.join(IO.ROOT, "textslam_amd", "libtsorb.so")):
        ge.build()
    exe = IO.build(tmp_path)
    c = IO.run(exe, str(tmp_path / "out.bin"), host=True)
    IO.check_counters(c)
    rec = IO.read_records(str(tmp_path / "out.bin"))
    for pre, n_set in (("fuse_", 4), ("more_", 1)):
        nq = len(rec[pre + "qset"])
        assert len(rec[pre + "foff"]) == n_set + 1 and len(rec[pre + "bounds"]) == 4 * n_set and len(rec[pre + "kp6"]) == 6 * rec[pre + "foff"][-1]
        assert nq == c["queries" if pre == "fuse_" else "mm_queries"] and len(rec[pre + "best_idx"]) == nq and len(rec[pre + "qxy"]) == 2 * nq
        assert (rec[pre + "cand_cnt"] > 0).any() and (rec[pre + "cand_cnt"] == 0).any()
    assert (rec["fuse_foff"][1:] - rec["fuse_foff"][:-1] >= 300).all()                # 4 keyframes of about 300 features
    assert (rec["fuse_qr"] == np.float32(15.0)).all() and (rec["more_qr"] == np.float32(15.0) * np.float32(1.2)).all()
