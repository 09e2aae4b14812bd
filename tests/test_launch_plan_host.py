"""The launch plan of a transition (irbpp_amd/csrc/irbpp_plan.h: plan_transition), compiled for the host by
tests/host/launch_plan_host.cpp: a pure function of Params, the tuning word and the call, so every launch decision can be
pinned without a device -- one row on each side of every size threshold, every key and mode, the tunings that change the shape
of the pipeline.  The expected launches below were written out by hand from the launcher as it stood before the plan existed
(launch_group / launch_apply of irbpp_capi.hip); the LDS sizes {lds} {full} {emit} are irbpp::layout_lds's, which the program
prints per geometry."""
import os
import shutil
import subprocess

import pytest

import irbpp_amd  # noqa: F401
from irbpp_amd import _lib as T

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "host", "launch_plan_host.cpp")
EXE = os.path.join(HERE, "host", "_build", "launch_plan_host")

RESET, STEP, CANDS, POSSIBLE, OBSERVE = 0, 1, 2, 3, 4          # irbpp_device.h: Mode
CAND, CELLS, HEUR, HEUR_HM = 0, 1, 2, 3                        # ApplyKey; 3: the heuristic step with method 4 (HM)
NONE, TRACK, FORGET = 0, 1, 2                                  # Plan::obs_rows
CHAIN_EXTRA = 5120                                             # S = 500: 10 bytes per entry of the next power of two


def row(geom, N, want, facts=None, K=1, stab=0, tuning=0, mode=STEP, n=None, key=CAND, listed=0, reg=0, turn=0, order=0):
    return (f"{geom} {N} {K} {stab} {tuning} {mode} {N if n is None else n} {key} {listed} {reg} {turn} {order}", want, facts or {})


def env(name, grid, mode, block=256):      # transition kernel: dynamic LDS = the tile's carve-up
    return f"irbpp_env_kernel{name} {grid} {block} {{lds}} {mode}"


def trace(sfx, grid, mode):
    return f"irbpp_trace_kernel{sfx} {grid} 64 0 {mode}"


def poly(grid, mode):
    return f"irbpp_polygon_kernel {grid} 64 0 {mode}"


def emit(name, grid, mode):                # name: "_s1", "_wave_s1", ...
    return f"irbpp_emit{name.replace('_wave', '_wave_kernel') if '_wave' in name else '_kernel' + name} {grid} 256 {{emit}} {mode}"


def apply(name, grid):                     # name: "", "_wg", "_cells", "_cells_wg", "_heur", "_heur_wg"
    return f"irbpp_apply{name}_kernel {grid} 256 0 1"


ROWS = [
    # trace candidates per wave: 32 up to 1024 bins, 64 beyond
    row("s1", 1024, [env("_s1", 1024, 1), trace("_c32", 2048, 1), poly(2048, 1), emit("_s1", 1024, 1)]),
    row("s1", 1025, [env("_s1", 1025, 1), trace("", 1025, 1), poly(2050, 1), emit("_s1", 1025, 1)]),
    # wave emit on lattice data from 2048 bins on; IRBPP_TUNE_BLOCK_EMIT / _WAVE_EMIT force either form
    row("s1", 2047, [env("_s1", 2047, 1), trace("", 2047, 1), poly(4094, 1), emit("_s1", 2047, 1)]),
    row("s1", 2048, [env("_s1", 2048, 1), trace("", 2048, 1), poly(4096, 1), emit("_wave_s1", 512, 1)]),
    row("s1", 2048, [env("_s1", 2048, 1), trace("", 2048, 1), poly(4096, 1), emit("_s1", 2048, 1)], tuning=T.TUNE_BLOCK_EMIT),
    row("s1", 2047, [env("_s1", 2047, 1), trace("", 2047, 1), poly(4094, 1), emit("_wave_s1", 512, 1)], tuning=T.TUNE_WAVE_EMIT),
    row("s1", 2047, [env("_s1", 2047, 1), trace("", 2047, 1), poly(4094, 1), emit("_s1", 2047, 1)], tuning=T.TUNE_BLOCK_EMIT),
    row("s1", 2048, [env("_s1", 2048, 1), trace("", 2048, 1), poly(4096, 1), emit("_wave_s1", 512, 1)], tuning=T.TUNE_WAVE_EMIT),
    # split_apply, lattice and box data: from 4096 bins on (the emit kernel keeps the caller's mode)
    row("s1", 4095, [env("_s1", 4095, 1), trace("", 4095, 1), poly(8190, 1), emit("_wave_s1", 1024, 1)], {"obs_rows": TRACK}, reg=1),
    row("s1", 4096, [apply("", 1024), env("_s1", 4096, 4), trace("", 4096, 1), poly(8192, 1), emit("_wave_s1", 1024, 1)], {"obs_rows": TRACK}, reg=1),
    row("s2", 4095, [env("_s2", 4095, 1), trace("", 4095, 1), poly(8190, 1), emit("_wave_s2", 1024, 1)]),
    row("s2", 4096, [apply("", 1024), env("_s2", 4096, 4), trace("", 4096, 1), poly(8192, 1), emit("_wave_s2", 1024, 1)]),
    row("s1", 1024, [apply("", 256), env("_s1", 1024, 4), trace("_c32", 2048, 1), poly(2048, 1), emit("_s1", 1024, 1)], tuning=T.TUNE_SPLIT_APPLY),
    row("s1", 8192, [env("_s1", 8192, 1), trace("", 8192, 1), poly(16384, 1), emit("_wave_s1", 2048, 1)], tuning=T.TUNE_FUSED_APPLY),
    row("s1", 4096, [env("", 4096, 1), trace("", 4096, 1), poly(8192, 1), emit("_wave", 1024, 1)], stab=1),       # (stability: fused, run-time builds)
    # ... cell lists where eight workgroups share a CU: from 8192 bins on (heavy-first: heavy_cap = N / 8 more emit workgroups)
    row("s3", 8191, [env("_s3", 8191, 1), trace("", 8191, 1), poly(16382, 1), emit("_s3", 8191 + 1023, 1)], {"heavy_first": 1, "heavy_turn": 0}),
    row("s3", 8192, [apply("", 2048), env("_s3", 8192, 4), trace("", 8192, 1), poly(16384, 1), emit("_s3", 8192 + 1024, 1)],
        {"heavy_first": 1, "heavy_turn": 1}, turn=1),
    row("s5", 8191, [env("_s5", 8191, 1), trace("", 8191, 1), poly(16382, 1), emit("_wave_s5", 2048, 1)], {"heavy_first": 0, "heavy_turn": -1}),
    row("s5", 8192, [apply("", 2048), env("_s5", 8192, 4), trace("", 8192, 1), poly(16384, 1), emit("_wave_s5", 2048, 1)]),
    # ... a tile that lets fewer than eight workgroups onto a CU (40 KB): never
    row("s4", 16384, [env("_s4_w512c", 16384, 1, 512), trace("", 16384, 1), poly(32768, 1), emit("_s4", 16384 + 2048, 1)], {"heavy_first": 1}),
    # _w512 below 4096 bins of the environment, _w512c from there on
    row("s4", 4095, [env("_s4_w512", 4095, 1, 512), trace("", 4095, 1), poly(8190, 1), emit("_s4", 4095 + 511, 1)]),
    row("s4", 4096, [env("_s4_w512c", 4096, 1, 512), trace("", 4096, 1), poly(8192, 1), emit("_s4", 4096 + 512, 1)]),
    row("s4", 4096, [env("_s4", 4096, 1), trace("", 4096, 1), poly(8192, 1), emit("_s4", 4096 + 512, 1)], tuning=T.TUNE_NO_WG512),
    row("s4", 96, [env("_generic_w512", 96, 1, 512), trace("_c32", 192, 1), poly(192, 1), emit("", 96 + 12, 1)], tuning=T.TUNE_NO_SPECIALISED),
    # buffered step: the apply kernel alone, a workgroup per bin below 2048 bins, a wave per bin from there on
    row("s1", 2047, [apply("_wg", 2047)], {"obs_rows": FORGET}, K=10, reg=1),
    row("s1", 2048, [apply("", 512)], {"obs_rows": NONE}, K=10),
    row("s1", 1024, [env("_s1", 1024, 1)], K=10, tuning=T.TUNE_FUSED_APPLY),
    row("s2", 1024, [apply("_wg", 1024)], K=10),
    # keys: the caller's cells, the heuristic's choice fused into the placing wave, HM's scorer in front of the cells apply
    row("s1", 1024, [apply("_cells", 256), env("_s1", 1024, 4), trace("_c32", 2048, 1), poly(2048, 1), emit("_s1", 1024, 1)], key=CELLS),
    row("s1", 1024, [apply("_heur", 256), env("_s1", 1024, 4), trace("_c32", 2048, 1), poly(2048, 1), emit("_s1", 1024, 1)], key=HEUR),
    row("s1", 1024, ["irbpp_heuristic_kernel 1024 256 {full} 1", apply("_cells", 256), env("_s1", 1024, 4), trace("_c32", 2048, 1),
                     poly(2048, 1), emit("_s1", 1024, 1)], key=HEUR_HM),
    row("s1", 1024, [apply("_cells_wg", 1024)], K=10, key=CELLS),
    row("s1", 2048, [apply("_heur", 512)], K=10, key=HEUR),
    row("s1", 1024, ["irbpp_heuristic_kernel 1024 256 {full} 1", apply("_cells_wg", 1024)], K=10, key=HEUR_HM),
    # modes
    row("s1", 1024, [env("_s1", 1024, 0), trace("_c32", 2048, 0), poly(2048, 0), emit("_s1", 1024, 0)], {"obs_rows": TRACK}, mode=RESET, reg=1),
    row("s3", 1024, [env("_s3", 100, 0), trace("_c32", 200, 0), poly(200, 0), emit("_s3", 100, 0)],
        {"heavy_first": 0, "heavy_turn": -1, "obs_rows": FORGET}, mode=RESET, n=100, listed=1, reg=1, turn=1),
    row("s3", 1024, [env("_s3", 1024, 0), trace("_c32", 2048, 0), poly(2048, 0), emit("_s3", 1024 + 128, 0)],
        {"heavy_first": 1, "heavy_turn": 1, "use_order": 0}, mode=RESET, turn=1, order=1),
    row("s1", 1024, [env("_s1", 1024, 0)], {"obs_rows": FORGET}, K=10, mode=RESET, reg=1),
    row("s1", 1024, [env("_s1", 1024, 2), trace("_c32", 2048, 2), poly(2048, 2), emit("_s1", 1024, 2)], {"obs_rows": TRACK}, K=10, mode=CANDS, reg=1),
    row("s2", 2048, [env("_s2", 2048, 2), trace("", 2048, 2), poly(4096, 2), emit("_wave_s2", 512, 2)], K=10, mode=CANDS),
    row("s1", 1024, [env("_s1", 1024, 3)], {"obs_rows": NONE}, mode=POSSIBLE),
    row("s1", 1024, [env("_s1", 1024, 3)], K=10, mode=POSSIBLE),
    # IRBPP_TUNE_CHAIN: one kernel per observation up to a 32 KB tile ...
    row("s1", 1024, [f"irbpp_env_kernel_chain_s1 1024 256 {15328 + CHAIN_EXTRA} 1"], tuning=T.TUNE_CHAIN),
    row("s1", 1024, [f"irbpp_env_kernel_chain_s1 1024 256 {15328 + CHAIN_EXTRA} 0"], tuning=T.TUNE_CHAIN, mode=RESET),
    row("s1", 1024, [env("_s1", 1024, 3)], tuning=T.TUNE_CHAIN, mode=POSSIBLE),
    row("s3", 8192, [f"irbpp_env_kernel_chain 8192 256 {18128 + CHAIN_EXTRA} 1"], {"heavy_first": 0, "heavy_turn": -1}, tuning=T.TUNE_CHAIN),
    row("s1@32768", 1024, [f"irbpp_env_kernel_chain 1024 256 {32768 + CHAIN_EXTRA} 1"], tuning=T.TUNE_CHAIN),
    row("s1@32784", 1024, ["irbpp_env_kernel_wide 1024 256 32784 1", trace("_c32", 2048, 1), poly(2048, 1), emit("", 1024, 1)], tuning=T.TUNE_CHAIN),
    # ... a buffered environment: the observation of get_action_candidates is the chain kernel, the step the apply kernel by size
    row("s1", 1024, [f"irbpp_env_kernel_chain_s1 1024 256 {15328 + CHAIN_EXTRA} 2"], K=10, tuning=T.TUNE_CHAIN, mode=CANDS),
    row("s1", 1024, [apply("_wg", 1024)], K=10, tuning=T.TUNE_CHAIN),
    row("s1", 2048, [apply("", 512)], K=10, tuning=T.TUNE_CHAIN),
    # ... and cancelled by the stability proxy and by every tuning that forces a shape of the split pipeline
    row("s1", 1024, [env("", 1024, 1), trace("_c32", 2048, 1), poly(2048, 1), emit("", 1024, 1)], tuning=T.TUNE_CHAIN, stab=1),
    row("s1", 1024, [env("_s1", 1024, 1), trace("", 1024, 1), poly(2048, 1), emit("_s1", 1024, 1)], tuning=T.TUNE_CHAIN | T.TUNE_TRACE_CPW64),
    row("s1", 1024, [env("_s1", 1024, 1), trace("_c32", 2048, 1), poly(2048, 1), emit("_s1", 1024, 1)], tuning=T.TUNE_CHAIN | T.TUNE_TRACE_CPW32),
    row("s1", 1024, [env("_s1", 1024, 1), trace("_c16", 4096, 1), poly(2048, 1), emit("_s1", 1024, 1)], tuning=T.TUNE_CHAIN | T.TUNE_TRACE_CPW16),
    row("s1", 1024, [env("_s1", 1024, 1), trace("_refill", 512, 1), poly(2048, 1), emit("_s1", 1024, 1)], tuning=T.TUNE_CHAIN | T.TUNE_TRACE_REFILL),
    row("s1", 1024, [env("_s1", 1024, 1), trace("_c32", 2048, 1), emit("_s1", 1024, 1)], {"inline_polygon": 1}, tuning=T.TUNE_CHAIN | T.TUNE_INLINE_POLYGON),
    row("s1", 1024, [env("_s1", 1024, 1), trace("_c32", 2048, 1), poly(2048, 1), emit("_s1", 1024, 1)], tuning=T.TUNE_CHAIN | T.TUNE_BLOCK_EMIT),
    row("s1", 1024, [env("_s1", 1024, 1), trace("_c32", 2048, 1), poly(2048, 1), emit("_wave_s1", 256, 1)], tuning=T.TUNE_CHAIN | T.TUNE_WAVE_EMIT),
    row("s1", 1024, [apply("", 256), env("_s1", 1024, 4), trace("_c32", 2048, 1), poly(2048, 1), emit("_s1", 1024, 1)], tuning=T.TUNE_CHAIN | T.TUNE_SPLIT_APPLY),
    row("s1", 1024, [env("_s1", 1024, 1), trace("_c32", 2048, 1), poly(2048, 1), emit("_s1", 1024, 1)], tuning=T.TUNE_CHAIN | T.TUNE_GRAPH),
    row("s1", 1024, [env("_s1", 1024, 1), trace("_c32", 2048, 1), poly(2048, 1), emit("_s1", 1024, 1)], tuning=T.TUNE_CHAIN | T.TUNE_WG512),
    row("s1", 1024, [env("", 1024, 1), trace("_c32", 2048, 1), poly(2048, 1), emit("", 1024, 1)], tuning=T.TUNE_CHAIN | T.TUNE_NARROW_KERNEL),
    # further tunings
    row("s1", 1024, [env("_s1_w128", 1024, 1, 128), trace("_c32", 2048, 1), poly(2048, 1), emit("_s1", 1024, 1)], tuning=T.TUNE_WG128),
    row("s2", 1024, [env("_s2", 1024, 1), trace("_c32", 2048, 1), poly(2048, 1), emit("_s2", 1024, 1)], tuning=T.TUNE_WG128),
    row("s1", 2048, [env("_s1", 2048, 1), trace("_refill", 1024, 1), poly(4096, 1), emit("_wave_s1", 512, 1)], tuning=T.TUNE_TRACE_REFILL),
    row("s1", 2048, [env("_s1", 2048, 1), trace("", 2048, 1), emit("_wave_s1", 512, 1)], {"inline_polygon": 1}, tuning=T.TUNE_INLINE_POLYGON),
    row("s3", 1024, [env("_s3", 1024, 1), trace("_c32", 2048, 1), poly(2048, 1), emit("_s3", 1024, 1)], {"heavy_first": 0, "heavy_turn": -1},
        tuning=T.TUNE_NO_HEAVY_FIRST, turn=1),
    # heavy-first: free-form level images only; the list of the environment's turn; N / 8 more emit workgroups; not below 64 bins
    row("s3", 1024, [env("_s3", 1024, 1), trace("_c32", 2048, 1), poly(2048, 1), emit("_s3", 1024 + 128, 1)], {"heavy_first": 1, "heavy_turn": 0}, turn=0),
    row("s3", 1024, [env("_s3", 1024, 1), trace("_c32", 2048, 1), poly(2048, 1), emit("_s3", 1024 + 128, 1)], {"heavy_first": 1, "heavy_turn": 1}, turn=1),
    row("s3", 63, [env("_s3", 63, 1), trace("_c32", 126, 1), poly(126, 1), emit("_s3", 63, 1)], {"heavy_first": 0, "heavy_turn": -1}, turn=1),
    row("s1", 1024, [env("_s1", 1024, 1), trace("_c32", 2048, 1), poly(2048, 1), emit("_s1", 1024, 1)], {"heavy_first": 0, "heavy_turn": -1}, turn=1),
    # online steps of a data set that launches its bins grouped by observed item
    row("s3", 4096, ["irbpp_item_order_kernel 1 1024 0 1", env("_s3", 4096, 1), trace("", 4096, 1), poly(8192, 1), emit("_s3", 4096 + 512, 1)],
        {"use_order": 1}, order=1),
    # geometries without a specialised build: free-form footprints, solid boxes, lattice footprints
    row("generic12", 1024, [env("_generic8", 1024, 1), trace("_c32", 2048, 1), poly(2048, 1), emit("", 1024 + 128, 1)], {"heavy_first": 1}),
    row("generic12", 1024, [env("_generic", 1024, 1), trace("_c32", 2048, 1), poly(2048, 1), emit("", 1024 + 128, 1)], tuning=T.TUNE_WIDE_KERNEL),
    row("box12", 2048, [env("_box8", 2048, 1), trace("", 2048, 1), poly(4096, 1), emit("_wave", 512, 1)]),
    row("lattice12", 4096, [apply("", 1024), env("", 4096, 4), trace("", 4096, 1), poly(8192, 1), emit("_wave", 1024, 1)]),
    # the capacity path: [the apply kernel,] then one kernel per observation (its LDS bytes are the executor's: -1)
    row("wide20", 96, [apply("", 24), "irbpp_wide_kernel 96 256 -1 4"], {"obs_rows": TRACK}, reg=1),
    row("wide20", 96, [apply("_cells", 24), "irbpp_wide_kernel 96 256 -1 4"], key=CELLS),
    row("wide20", 96, ["irbpp_wide_kernel 96 256 -1 0"], mode=RESET),
    row("wide20", 96, [apply("_wg", 96)], {"obs_rows": FORGET}, K=3, reg=1),
    row("wide20", 2048, [apply("", 512)], K=3),
    row("wide20", 96, ["irbpp_wide_kernel 96 256 -1 2"], K=3, mode=CANDS),
    row("wide20", 96, ["irbpp_wide_kernel 96 256 -1 0"], K=3, mode=RESET),
    # the trace grid never exceeds the scratch the environment allocated: max(N, min(4 N, 8192)) waves
    row("s1", 2048, [env("_s1", 2048, 1), trace("_c16", 8192, 1), poly(4096, 1), emit("_wave_s1", 512, 1)], tuning=T.TUNE_TRACE_CPW16),
    row("s1", 2049, [env("_s1", 2049, 1), trace("_c16", 8192, 1), poly(4098, 1), emit("_wave_s1", 513, 1)], tuning=T.TUNE_TRACE_CPW16),
    row("s1", 4096, [apply("", 1024), env("_s1", 4096, 4), trace("_c16", 8192, 1), poly(8192, 1), emit("_wave_s1", 1024, 1)], tuning=T.TUNE_TRACE_CPW16),
    row("s1", 4096, [apply("", 1024), env("_s1", 4096, 4), trace("_c32", 8192, 1), poly(8192, 1), emit("_wave_s1", 1024, 1)], tuning=T.TUNE_TRACE_CPW32),
    row("s1", 4097, [apply("", 1025), env("_s1", 4097, 4), trace("_c32", 8192, 1), poly(8194, 1), emit("_wave_s1", 1025, 1)], tuning=T.TUNE_TRACE_CPW32),
    row("s1", 16384, [apply("", 4096), env("_s1", 16384, 4), trace("_c32", 16384, 1), poly(32768, 1), emit("_wave_s1", 4096, 1)], tuning=T.TUNE_TRACE_CPW32),
    row("s1", 4, [env("_s1", 4, 1), trace("_c32", 8, 1), poly(8, 1), emit("_s1", 4, 1)]),
    # a launch over some of the bins (a listed reset) goes by ITS size
    row("s1", 8192, [env("_s1", 2047, 0), trace("", 2047, 0), poly(4094, 0), emit("_s1", 2047, 0)], mode=RESET, n=2047, listed=1),
    row("s1", 8192, [env("_s1", 1024, 0), trace("_c32", 2048, 0), poly(2048, 0), emit("_s1", 1024, 0)], mode=RESET, n=1024, listed=1),
    # registered observation buffers (tests/test_gpu_registered_obs.py plays these): a launch that observes all bins tracks the
    # row counts whatever the key, the form of the emit stage or the tuning; one that writes another layout through the
    # pointer (a listed reset, a buffered step / reset) forgets them
    row("s1", 1024, [apply("_cells", 256), env("_s1", 1024, 4), trace("_c32", 2048, 1), poly(2048, 1), emit("_s1", 1024, 1)],
        {"obs_rows": TRACK}, key=CELLS, reg=1),
    row("s1", 1024, [apply("_heur", 256), env("_s1", 1024, 4), trace("_c32", 2048, 1), poly(2048, 1), emit("_s1", 1024, 1)],
        {"obs_rows": TRACK}, key=HEUR, reg=1),
    row("s1", 1024, ["irbpp_heuristic_kernel 1024 256 {full} 1", apply("_cells", 256), env("_s1", 1024, 4), trace("_c32", 2048, 1),
                     poly(2048, 1), emit("_s1", 1024, 1)], {"obs_rows": TRACK}, key=HEUR_HM, reg=1),
    row("s1", 1024, [apply("_cells_wg", 1024)], {"obs_rows": FORGET}, K=10, key=CELLS, reg=1),
    row("s1", 2048, [apply("_heur", 512)], {"obs_rows": FORGET}, K=10, key=HEUR, reg=1),
    row("s1", 1024, [f"irbpp_env_kernel_chain_s1 1024 256 {15328 + CHAIN_EXTRA} 1"], {"obs_rows": TRACK}, tuning=T.TUNE_CHAIN, reg=1),
    row("s1", 1024, [f"irbpp_env_kernel_chain_s1 1024 256 {15328 + CHAIN_EXTRA} 0"], {"obs_rows": TRACK}, tuning=T.TUNE_CHAIN, mode=RESET, reg=1),
    row("s1", 1024, [f"irbpp_env_kernel_chain_s1 1024 256 {15328 + CHAIN_EXTRA} 2"], {"obs_rows": TRACK}, K=10, tuning=T.TUNE_CHAIN, mode=CANDS, reg=1),
    row("s1", 1024, [apply("_wg", 1024)], {"obs_rows": FORGET}, K=10, tuning=T.TUNE_CHAIN, reg=1),
    row("s1", 64, [env("_s1", 64, 1), trace("_c32", 128, 1), poly(128, 1), emit("_s1", 64, 1)], {"obs_rows": TRACK}, tuning=T.TUNE_GRAPH, reg=1),
    row("s1", 64, [env("_s1", 64, 1), trace("_c32", 128, 1), poly(128, 1), emit("_wave_s1", 16, 1)], {"obs_rows": TRACK},
        tuning=T.TUNE_GRAPH | T.TUNE_WAVE_EMIT, reg=1),
    row("s1", 67, [env("_s1", 67, 1), trace("_c32", 134, 1), poly(134, 1), emit("_wave_s1", 17, 1)], {"obs_rows": TRACK}, tuning=T.TUNE_WAVE_EMIT, reg=1),
    row("s1", 67, [env("_s1", 67, 0), trace("_c32", 134, 0), poly(134, 0), emit("_wave_s1", 17, 0)], {"obs_rows": TRACK},
        tuning=T.TUNE_WAVE_EMIT, mode=RESET, reg=1),
    row("s1", 35, [env("_s1", 35, 2), trace("_c32", 70, 2), poly(70, 2), emit("_wave_s1", 9, 2)], {"obs_rows": TRACK}, K=10,
        tuning=T.TUNE_WAVE_EMIT, mode=CANDS, reg=1),
    # ... a listed reset (a row per LISTED bin), then the step into the same buffer
    row("s1", 67, [env("_s1", 22, 0), trace("_c32", 44, 0), poly(44, 0), emit("_wave_s1", 6, 0)], {"obs_rows": FORGET},
        tuning=T.TUNE_WAVE_EMIT, mode=RESET, n=22, listed=1, reg=1),
    row("s1", 67, [env("_s1", 22, 0), trace("_c32", 44, 0), poly(44, 0), emit("_s1", 22, 0)], {"obs_rows": FORGET},
        tuning=T.TUNE_BLOCK_EMIT, mode=RESET, n=22, listed=1, reg=1),
    row("s1", 67, [env("_s1", 67, 1), trace("_c32", 134, 1), poly(134, 1), emit("_s1", 67, 1)], {"obs_rows": TRACK}, tuning=T.TUNE_BLOCK_EMIT, reg=1),
    # ... the capacity path, online and buffered (K > 1)
    row("wide20", 96, [apply("_heur", 24), "irbpp_wide_kernel 96 256 -1 4"], {"obs_rows": TRACK}, key=HEUR, reg=1),
    row("wide20", 96, ["irbpp_wide_kernel 96 256 -1 0"], {"obs_rows": TRACK}, mode=RESET, reg=1),
    row("wide20", 96, ["irbpp_wide_kernel 30 256 -1 0"], {"obs_rows": FORGET}, mode=RESET, n=30, listed=1, reg=1),
    row("wide20", 96, ["irbpp_wide_kernel 96 256 -1 2"], {"obs_rows": TRACK}, K=3, mode=CANDS, reg=1),
    row("wide20", 96, ["irbpp_wide_kernel 96 256 -1 0"], {"obs_rows": FORGET}, K=3, mode=RESET, reg=1),
    row("wide20", 96, [apply("_cells_wg", 96)], {"obs_rows": FORGET}, K=3, key=CELLS, reg=1),
    row("wide20", 2048, [apply("", 512)], {"obs_rows": FORGET}, K=3, reg=1),
]


@pytest.fixture(scope="module")
def plans():
    if shutil.which("g++") is None:
        pytest.skip("no host compiler")
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Werror", "-I", os.path.join(HERE, "host", "stub"), SRC, "-o", EXE], check=True)
    res = subprocess.run([EXE], input="".join(r[0] + "\n" for r in ROWS), capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-400:] + res.stderr
    blocks = res.stdout.split("end\n")[:-1]
    assert len(blocks) == len(ROWS)
    return blocks


@pytest.mark.parametrize("i", range(len(ROWS)), ids=[r[0].replace(" ", "-") for r in ROWS])
def test_plan(plans, i):
    request, want, facts = ROWS[i]
    lines = plans[i].strip().split("\n")
    layout = dict(kv.split("=") for kv in lines[0].split()[1:])
    got_facts = {k: int(v) for k, v in (kv.split("=") for kv in lines[-1].split()[1:])}
    assert lines[1:-1] == [w.format(**layout) for w in want], request
    for name, value in facts.items():
        assert got_facts[name] == value, (request, name)
    # what follows from the launches, in every row
    kernels = [ln.split()[0] for ln in lines[1:-1]]
    assert got_facts["inline_polygon"] == int(any("trace" in k for k in kernels) and "irbpp_polygon_kernel" not in kernels)
    assert got_facts["use_order"] == int(kernels[0] == "irbpp_item_order_kernel")
    assert (got_facts["heavy_turn"] >= 0) == bool(got_facts["heavy_first"])
