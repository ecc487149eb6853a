"""Calls that concern the device or a launch plan and no world: device queries, the clock probe and sampler, the preflight
checks of the sharded start-up, and the host arithmetic of the launch policy."""
import ctypes as C

from ._abi import UNIQUE_ID_BYTES, NbShardPlan, hip_lib


def device_count():
    return int(hip_lib().nb_hip_device_count())


def live_resources():
    """nb_hip_live_resources (tuning hook): (device allocations, events) the library holds right now; needs no GPU."""
    buffers, events = C.c_uint32(0), C.c_uint32(0)
    hip_lib().nb_hip_live_resources(C.byref(buffers), C.byref(events))
    return int(buffers.value), int(events.value)


def device_info():
    buf = C.create_string_buffer(256)
    hip_lib().nb_hip_device_info(buf, 256)
    return buf.value.decode()


def probe_clock(target_ms=40.0):
    """include/nbody_hip.h nb_hip_probe_clock: the shader clock held under the step kernels' instruction mix."""
    v = [C.c_double(0.0) for _ in range(5)]
    waves = hip_lib().nb_hip_probe_clock(float(target_ms), *[C.byref(x) for x in v])
    return {"clock_ghz": v[0].value, "clock_ghz_min": v[1].value, "clock_ghz_max": v[2].value,
            "cycles_per_wave_interaction": v[3].value, "elapsed_ms": v[4].value, "waves": int(waves)}


def clock_sampler_begin(period_ms=0.5, max_ms=6000.0):
    """include/nbody_hip.h nb_hip_clock_sampler_begin: sample the shader clock while other kernels run."""
    return int(hip_lib().nb_hip_clock_sampler_begin(float(period_ms), float(max_ms)))


def clock_sampler_end():
    ghz, lo, hi, span = C.c_double(), C.c_double(), C.c_double(), C.c_double()
    per_xcd, profile = (C.c_double * 8)(), (C.c_double * 10)()
    dropped = C.c_uint32(0)
    n = hip_lib().nb_hip_clock_sampler_end(C.byref(ghz), C.byref(lo), C.byref(hi), per_xcd, profile, C.byref(span), C.byref(dropped))
    return {"clock_ghz": ghz.value, "clock_ghz_min": lo.value, "clock_ghz_max": hi.value, "per_xcd_ghz": [float(v) for v in per_xcd],
            "profile_ghz": [float(v) for v in profile], "span_ms": span.value, "intervals": int(n), "dropped_intervals": int(dropped.value)}


def preflight_peers(max_devices=16):
    """include/nbody_hip.h nb_hip_preflight_peers: (visible devices, hipDeviceCanAccessPeer row of this process' device)."""
    row = (C.c_int * max_devices)()
    count = int(hip_lib().nb_hip_preflight_peers(row, max_devices))
    return count, [int(v) for v in row[:min(count, max_devices)]]


def preflight_ipc_export(tag):
    """(hipError_t, 64-byte IPC handle of a device word holding `tag`)."""
    buf = (C.c_ubyte * 64)()
    rc = int(hip_lib().nb_hip_preflight_ipc_export(buf, int(tag) & 0xffffffff))
    return rc, bytes(buf)


def preflight_ipc_open(handle, expect_tag):
    """(0 / hipError_t / -1, host ms) of mapping a peer's exported word, reading it and unmapping."""
    ms = C.c_double(0.0)
    buf = (C.c_ubyte * 64).from_buffer_copy(handle)
    rc = int(hip_lib().nb_hip_preflight_ipc_open(buf, int(expect_tag) & 0xffffffff, C.byref(ms)))
    return rc, float(ms.value)


def hip_error_string(code):
    return hip_lib().nb_hip_error_string(int(code)).decode(errors="replace")


def shard_plan(total_len, mass_len, rank, nranks):
    p = hip_lib().nb_hip_shard_plan(total_len, mass_len, rank, nranks)
    return {n: int(getattr(p, n)) for n, _ in NbShardPlan._fields_}


def plan_launch(n_recv, n_src, compute_units=256):
    """The classic (k, w, split, unit) plan, plus "lanes" / "lanes_w": whether an all-auto unsharded step of that size
    runs as a lane-split launch instead (lanes > 1) and with how many waves per workgroup."""
    k, w, sp, g, lw = C.c_int(), C.c_int(), C.c_int(), C.c_uint32(), C.c_int()
    hip_lib().nb_hip_plan_launch(n_recv, n_src, compute_units, C.byref(k), C.byref(w), C.byref(sp), C.byref(g))
    lanes = int(hip_lib().nb_hip_plan_launch_lanes(n_recv, n_src, C.byref(lw)))
    return {"k": k.value, "w": w.value, "split": sp.value, "workgroups": g.value,
            "unit": int(hip_lib().nb_hip_plan_launch_unit(n_recv, n_src, compute_units)), "lanes": lanes, "lanes_w": lw.value,
            "fused_finish": int(hip_lib().nb_hip_plan_fused_finish(n_recv, n_src, compute_units))}


def plan_deal(n_recv, n_src, compute_units=256):
    """tuning hook: whether "deal" = 2 deals the step launches of an unsharded world of that size (host arithmetic)."""
    return bool(hip_lib().nb_hip_plan_deal(n_recv, n_src, compute_units))


def deal_item(ticket, tiles, split):
    """tuning hook: the (receiver tile, source part) a dealt launch's ticket stands for, or None past the last item."""
    tile, part = C.c_uint32(0), C.c_uint32(0)
    live = hip_lib().nb_hip_deal_item(ticket, tiles, split, C.byref(tile), C.byref(part))
    return (int(tile.value), int(part.value)) if live else None


def comm_unique_id():
    buf = (C.c_ubyte * UNIQUE_ID_BYTES)()
    hip_lib().nb_hip_comm_unique_id(buf)
    return bytes(buf)
