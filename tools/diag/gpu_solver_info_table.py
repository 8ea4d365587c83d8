"""What tsba_debug_solver_info reports for the maps the GPU suite uploads without a band_parts override: one line per map, the inputs of
choose_solver_layout (csrc/tsba_layout.h) on the left, what the upload chose on the right.  Run on two builds and diff the output
(profiles/upload_stages_solver_info_parent_vs_branch.txt; the rows are pinned in tests/test_solver_layout.py)."""
import os
import sys
import threading

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from textslam_amd import synth, abi                                    # noqa: E402
from textslam_amd.optimizer import Optimizer, local_group_create, local_group_destroy      # noqa: E402


def line(name, P, info, ring_k0=0, multi=0):
    print("%-28s n_kf %5d bw_rows %3d ring_plan %d ring_k0 %4d multi %d | lds %d band %d stream %d P %3d cr %d ring %d" % (
        name, P.n_kf, info["band_rows"], info["ring"], ring_k0, multi,
        info["lds_solver"], info["band_storage"], info["band_stream"], info["interiors"], info["sep_cr"], info["ring"]), flush=True)


def main():
    g = Optimizer(0)
    og = abi.options_global()
    P = synth.config_c4(); g.upload(P, abi.options_local()); line("c4_window_20", P, g.solver_info())
    for n_kf, n_pt, band in ((300, 8000, 8), (700, 20000, 9), (5000, 70000, 10)):
        P = synth.config_global(n_kf=n_kf, n_pt=n_pt, band=band); g.upload(P, og); line("global_%d_band_%d" % (n_kf, band), P, g.solver_info())
    P = synth.make_problem(n_kf=500, n_pt=50000, n_text=1000, seed=7, feats=(64, 24, 12), max_targets=8, text_targets=5, frozen_frac=0.0, band=12, n_levels=1,
                           rot_deg=0.2, trans_m=0.01)
    o = abi.options_global(); o.use_text = 1; g.upload(P, o); line("c5_500_text", P, g.solver_info())
    for n_kf, band in ((600, 8), (2400, 11)):
        P = synth.config_global(n_kf=n_kf, n_pt=30*n_kf, band=band, loop=True); g.upload(P, og); line("ring_%d_band_%d" % (n_kf, band), P, g.solver_info())
    for n_kf, k0, band in ((600, 200, 8), (1500, 1000, 7)):
        P = synth.config_global(n_kf=n_kf, n_pt=20*n_kf, band=band, loop=True, loop_at=k0); g.upload(P, og); line("tail_%d_at_%d" % (n_kf, k0), P, g.solver_info(), ring_k0=k0)
    P = synth.config_global(n_kf=600, n_pt=12000, band=8, far_frac=0.02)
    g.debug_set(far_solver=2); g.upload(P, og); line("far_600 (far_solver=2)", P, g.solver_info()); g.debug_set()
    g.close()
    # world = 2 on one device (in-process communicator): every rank derives the same layout
    P = synth.config_global(n_kf=300, n_pt=9000, band=8); group = local_group_create(2); out = [None, None]

    def run(rank):
        r = Optimizer(0); r.comm_init_local(group, rank, 2); r.upload(P, og); out[rank] = r.solver_info(); r.close()
    th = [threading.Thread(target=run, args=(r,)) for r in range(2)]
    for t in th:
        t.start()
    for t in th:
        t.join(600)
    local_group_destroy(group)
    for r in range(2):
        line("world2_300 rank %d" % r, P, out[r], multi=1)


if __name__ == "__main__":
    main()
