"""ctypes binding of libstrique_hip.so (include/strique_hip.h).

This is the only place the package touches the native library.  There is no CPU fallback:
if the library is missing or no GPU is present, creating a `Context` raises.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("STRQ_LIB") or os.path.join(_HERE, "lib", "libstrique_hip.so")      # STRQ_LIB: A/B testing of builds

STRQ_OK, STRQ_ERR_ARG, STRQ_ERR_DEVICE, STRQ_ERR_UNSUPPORTED, STRQ_ERR_NOMEM = 0, 1, 2, 3, 4

SCAN_SYMBOLS = ("strq_scan_batch_reads", "strq_scan_set", "strq_scan_clear", "strq_batch_fetch_scan")

_lib = None


class StriqueHipError(RuntimeError):
    def __init__(self, code, message):
        RuntimeError.__init__(self, "libstrique_hip error %d: %s" % (code, message))
        self.code = code


def _torch_hip_runtime():
    """Path of the HIP runtime a PyTorch-ROCm wheel bundles (torch/lib/libamdhip64.so), found WITHOUT importing torch."""
    import importlib.util
    try:
        spec = importlib.util.find_spec("torch")
    except (ImportError, ValueError):
        spec = None
    if spec is None or not spec.submodule_search_locations:
        return None
    cand = os.path.join(list(spec.submodule_search_locations)[0], "lib", "libamdhip64.so")
    return cand if os.path.exists(cand) else None


def mapped_hip_runtimes():
    """Files of every HIP runtime mapped into this process (diagnostics, tests): there must never be two."""
    seen = set()
    try:
        for line in open("/proc/self/maps"):
            f = line.split()[-1]
            if "libamdhip64" in os.path.basename(f):
                seen.add(os.path.realpath(f))
    except OSError:
        pass
    return sorted(seen)


def _pin_hip_runtime():
    """One HIP runtime per process, whatever the import order.

    libstrique_hip.so needs `libamdhip64.so.7`; a PyTorch-ROCm wheel brings its own copy with the SAME soname.  If torch is
    imported first, the dynamic linker resolves the library's dependency to torch's already-loaded copy (soname match) and
    the process has one runtime.  The other order used to load /opt/rocm's copy here and torch's copy later -- two
    runtimes, and torch.cuda could no longer initialise (round 3's README note).  So the decision is taken here, before
    the library is opened: when a torch wheel with a bundled runtime is installed, that copy is loaded first (by path,
    RTLD_GLOBAL; torch itself is not imported), and both this library and a later `import torch` -- for RCCL through
    torch.distributed -- bind to it.  STRQ_HIP_RUNTIME=system keeps /opt/rocm's runtime (a process that never imports
    torch), STRQ_HIP_RUNTIME=/path/to/libamdhip64.so names one."""
    choice = os.environ.get("STRQ_HIP_RUNTIME", "auto")
    if choice == "system" or mapped_hip_runtimes():
        return None
    path = _torch_hip_runtime() if choice in ("auto", "torch") else choice
    if path is None:
        if choice == "torch":
            raise ImportError("STRQ_HIP_RUNTIME=torch: no torch wheel with a bundled libamdhip64.so found")
        return None
    ctypes.CDLL(path, mode=ctypes.RTLD_GLOBAL)
    return path


def load_library(path=None):
    """Load the shared library (building nothing: see strique_amd.build / __graft_entry__.build)."""
    global _lib
    if _lib is None:
        path = path or LIB_PATH
        if not os.path.exists(path):
            raise ImportError("%s not found: run `python -m strique_amd.build` (hipcc, gfx950) first" % path)
        _pin_hip_runtime()
        lib = ctypes.CDLL(path)
        lib.strq_last_error.restype = ctypes.c_char_p
        lib.strq_last_error.argtypes = [ctypes.c_void_p]
        lib.strq_ctx_destroy.restype = None
        lib.strq_ctx_destroy.argtypes = [ctypes.c_void_p]
        lib.strq_set_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p]
        lib.strq_get_option.argtypes = [ctypes.c_void_p, ctypes.c_char_p, ctypes.c_char_p, ctypes.c_int32]
        for name in SCAN_SYMBOLS:
            getattr(lib, name).restype = ctypes.c_int          # a library without the scan entries is an error here, not at the first scan
        _lib = lib
    return _lib


def _ptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def host_stats(signals, offsets, want_raw=False):
    """strq_host_stats: the six host-side scalars per float64 read (median, MAD, c1, h1 of the median-filtered signal;
    c1, h1 of the raw one), with numpy's arithmetic.  No context and no device involved."""
    lib = load_library()
    signals = _c(signals, np.float64); offsets = _c(offsets, np.int64)
    out = np.zeros((len(offsets) - 1, 6), np.float64)
    rc = lib.strq_host_stats(_ptr(signals), _ptr(offsets), ctypes.c_int64(len(offsets) - 1), ctypes.c_int32(1 if want_raw else 0), _ptr(out))
    if rc != STRQ_OK:
        raise StriqueHipError(rc, "strq_host_stats: bad argument")
    return out


def live_allocations():
    """strq_debug_live_allocations: (device blocks, pinned host blocks) the library holds in this process right now, over all
    contexts.  No context and no device involved."""
    out = np.zeros(2, np.int64)
    rc = load_library().strq_debug_live_allocations(_ptr(out))
    if rc != STRQ_OK:
        raise StriqueHipError(rc, "strq_debug_live_allocations: bad argument")
    return int(out[0]), int(out[1])


def _offsets(arrays, dtype):
    """Concatenation and int64 offsets of a list of arrays (one entry of at least one element, so that the pointer is never null)."""
    off = np.zeros(len(arrays) + 1, np.int64)
    for i, a in enumerate(arrays):
        off[i + 1] = off[i] + len(a)
    flat = np.concatenate([_c(a, dtype).ravel() for a in arrays] + [np.zeros(1, dtype)])
    return flat, off


# arrays of an edge image: name -> (dtype, shape), in the order of the hooks' offsets (csrc/variant_kernels.h, csrc/mod_llr_kernels.h)
_IMAGE_ORDER = ("src", "lp", "src2", "lp2", "start_lp", "kind", "hub", "ea", "eb", "ec", "end_src", "end_lp")
VARIANT_IMAGE_SHAPES = {"src": (np.int32, (2, 8, 64)), "lp": (np.float64, (2, 8, 64)), "src2": (np.int32, (3, 2, 4, 64)), "lp2": (np.float64, (3, 2, 4, 64)),
                        "start_lp": (np.float64, (2, 64)), "kind": (np.int32, (2, 64)), "hub": (np.int32, (2, 64)), "ea": (np.float64, (2, 64)),
                        "eb": (np.float64, (2, 64)), "ec": (np.float64, (2, 64)), "end_src": (np.int32, (4, 8)), "end_lp": (np.float64, (4, 8))}
MOD_LLR_IMAGE_SHAPES = dict(VARIANT_IMAGE_SHAPES, src2=(np.int32, (2, 4, 64)), lp2=(np.float64, (2, 4, 64)), start_lp=(np.float64, (2, 2, 64)),
                            end_src=(np.int32, (2, 8)), end_lp=(np.float64, (2, 8)))


def _debug_image(entry, shapes, baked, extra):
    lib = load_library()
    arrs = [_c(baked.in_ptr, np.int32), _c(baked.in_src, np.int32), _c(baked.in_logp, np.float64), _c(baked.emis_kind, np.int32),
            _c(baked.emis_a, np.float64), _c(baked.emis_b, np.float64), _c(baked.emis_c, np.float64),
            None if baked.tag is None else _c(baked.tag, np.int32)]
    brc = ctypes.c_int32(-1); head = np.zeros(10, np.int32); offs = np.zeros(12, np.int64); nbytes = ctypes.c_int64(0)
    image = np.zeros(1 << 16, np.uint8); why = ctypes.create_string_buffer(512)
    rc = getattr(lib, entry)(ctypes.c_int32(baked.n_states), ctypes.c_int32(baked.silent_start), ctypes.c_int32(baked.start), ctypes.c_int32(baked.end),
                             *([_ptr(a) for a in arrs] + extra + [ctypes.byref(brc), _ptr(head), _ptr(offs), _ptr(image), ctypes.c_int64(len(image)),
                                                                ctypes.byref(nbytes), why, ctypes.c_int32(512)]))
    if rc != STRQ_OK:
        raise StriqueHipError(rc, "%s: bad argument" % entry)
    out = {"rc": int(brc.value), "why": why.value.decode()}
    if brc.value:
        return out
    if nbytes.value > len(image):
        raise StriqueHipError(STRQ_ERR_NOMEM, "%s: an image of %d bytes" % (entry, nbytes.value))
    out.update(n_emit=int(head[0]), n_branch=int(head[1]), mode=int(head[2]), deg=int(head[3]), deg2=int(head[4]),
               end_deg=[int(v) for v in head[5:5 + int(head[1])]])
    for name, at in zip(_IMAGE_ORDER, offs):
        dtype, shape = shapes[name]
        count = int(np.prod(shape))
        out[name] = np.frombuffer(image.tobytes(), dtype, count, int(at)).reshape(shape).copy()
    return out


def debug_variant_image(baked, n_alt):
    """strq_debug_variant_image: the edge image of the variant pass for a baked model, as a dict -- 'rc' (0, or 1 with 'why': a model
    the pass does not cover), 'mode', 'n_branch', 'deg', 'deg2', 'end_deg' and the arrays of VARIANT_IMAGE_SHAPES.  No context, no device."""
    return _debug_image("strq_debug_variant_image", VARIANT_IMAGE_SHAPES, baked, [ctypes.c_int32(n_alt)])


def debug_mod_llr_image(baked):
    """strq_debug_mod_llr_image: the same for the per-unit scores of the modification pass (MOD_LLR_IMAGE_SHAPES)."""
    return _debug_image("strq_debug_mod_llr_image", MOD_LLR_IMAGE_SHAPES, baked, [])


VIT_COUNT, VIT_BACKPTR, VIT_MARK, VIT_HUB, VIT_UNIT = range(5)
VIT_SHAPE_CSR, VIT_SHAPE_G2, VIT_SHAPE_SS = 8, 9, 16
VIT_SRC_F64, VIT_SRC_F64_AFFINE, VIT_SRC_I16_AFFINE = 0, 1, 2          # how a window is given (csrc/vit_model.h)


def debug_viterbi_plan(baked):
    """strq_debug_viterbi_plan: the Viterbi kernel shape strq_model_create would put a baked model on, as a dict -- 'shape' (the id,
    16 added for a single-stage model, 8 = the general kernel), 'row', 'ss', 'modes' (the decode modes the library launches for it),
    'epl', 'spl', 'e_deg', 's_deg', 'e_flat', 'single_stage', 'silent_counted', 'rec_state', 'unit_state', 'csr'.  No context, no device."""
    lib = load_library()
    hints = getattr(baked, 'hint_slot', None) is not None and (np.asarray(baked.hint_slot)[:baked.silent_start] >= 0).all()
    arrs = [_c(baked.in_ptr, np.int32), _c(baked.in_src, np.int32), _c(baked.in_logp, np.float64), _c(baked.emis_kind, np.int32),
            _c(baked.emis_a, np.float64), _c(baked.emis_b, np.float64), _c(baked.emis_c, np.float64), _c(baked.count_inc, np.int32),
            None if baked.tag is None else _c(baked.tag, np.int32),
            _c(baked.hint_slot, np.int32) if hints else None, _c(baked.hint_lane, np.int32) if hints else None]
    out = np.zeros(48, np.int32); why = ctypes.create_string_buffer(256)
    rc = lib.strq_debug_viterbi_plan(ctypes.c_int32(baked.n_states), ctypes.c_int32(baked.silent_start), ctypes.c_int32(baked.start),
                                     ctypes.c_int32(baked.end), *([_ptr(a) for a in arrs] + [_ptr(out), why, ctypes.c_int32(256)]))
    if rc != STRQ_OK:
        raise StriqueHipError(rc, "strq_debug_viterbi_plan: " + why.value.decode())
    shape = int(out[0])
    epl, spl = int(out[10]), int(out[11])
    return {"shape": shape, "row": shape & ~VIT_SHAPE_SS if shape >= 0 else -1, "ss": bool(shape >= 0 and shape & VIT_SHAPE_SS),
            "shapes": [int(v) for v in out[0:5]], "modes": [m for m in range(5) if out[5 + m]], "epl": epl, "spl": spl,
            "e_deg": [int(v) for v in out[12:12 + epl]], "s_deg": [int(v) for v in out[20:20 + spl]], "e_flat": [int(v) for v in out[28:28 + epl]],
            "single_stage": int(out[36]), "silent_counted": int(out[37]), "rec_state": int(out[38]),
            "unit_state": (int(out[39]), int(out[40])), "csr": int(out[41])}


class Context(object):
    """One HIP context / stream / workspace on one GPU (strq_ctx)."""

    def __init__(self, device=0):
        self._lib = load_library()
        self._h = ctypes.c_void_p()
        rc = self._lib.strq_ctx_create(ctypes.c_int(device), ctypes.byref(self._h))
        if rc != STRQ_OK:
            self._h = None
            raise StriqueHipError(rc, "cannot create a context on HIP device %d (no GPU?)" % device)
        self.device = device

    def close(self):
        if getattr(self, "_h", None):
            self._lib.strq_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != STRQ_OK:
            raise StriqueHipError(rc, self._lib.strq_last_error(self._h).decode())

    def device_synchronize(self):
        self._check(self._lib.strq_device_synchronize(self._h))

    def set_option(self, key, value):
        """strq_set_option on this context: `value` None removes the entry (the process-wide table / the environment variable
        of the same name decide again), "" means "not set" whatever they say; anything else is stored as its str()."""
        v = None if value is None else str(value).encode()
        self._check(self._lib.strq_set_option(self._h, key.encode(), v))

    def get_option(self, key):
        """Effective value of a switch for this context ("" when unset)."""
        buf = ctypes.create_string_buffer(256)
        self._check(self._lib.strq_get_option(self._h, key.encode(), buf, ctypes.c_int32(256)))
        return buf.value.decode()

    # ---- alignment ------------------------------------------------------------------------
    def set_align_params(self, open_h, ext_h, open_v, ext_v, dist_offset, dist_min):
        p = np.array([open_h, ext_h, open_v, ext_v, dist_offset, dist_min], dtype=np.float32)
        self._check(self._lib.strq_set_align_params(self._h, _ptr(p)))

    def get_align_params(self):
        p = np.zeros(6, np.float32)
        self._check(self._lib.strq_get_align_params(self._h, _ptr(p)))
        return p

    def align_overlap(self, a, b, want_idx=True):
        """(score, a_idx, b_idx, rec, j_end, j0); inputs are rounded to float32 like the reference's
        pybind11 caster does (src/pyalign.cpp:59-61)."""
        a = _c(a, np.float32); b = _c(b, np.float32)
        n, m = len(a), len(b)
        score = ctypes.c_float(); j_end = ctypes.c_int64(); j0 = ctypes.c_int64()
        rec = np.zeros(m, np.int32)
        a_idx = np.zeros(n, np.uint64) if want_idx else None
        b_idx = np.zeros(m, np.uint64) if want_idx else None
        self._check(self._lib.strq_align_overlap(self._h, _ptr(a), ctypes.c_int64(n), _ptr(b), ctypes.c_int64(m),
                                                 ctypes.byref(score), _ptr(a_idx), _ptr(b_idx), _ptr(rec),
                                                 ctypes.byref(j_end), ctypes.byref(j0)))
        return score.value, a_idx, b_idx, rec, j_end.value, j0.value

    def align_batch(self, levels, read_off, level_val, align_read, flank, flank_off, samples=6, want_rec=True):
        levels = _c(levels, np.uint8); read_off = _c(read_off, np.int64); level_val = _c(level_val, np.float32)
        align_read = _c(align_read, np.int32); flank = _c(flank, np.float32); flank_off = _c(flank_off, np.int64)
        na, nr = len(align_read), len(read_off) - 1
        score = np.zeros(na, np.float32); j_end = np.zeros(na, np.int64); j0 = np.zeros(na, np.int64)
        rec = np.zeros(len(flank), np.int32) if want_rec else None
        self._check(self._lib.strq_align_batch(self._h, ctypes.c_int64(na), ctypes.c_int64(nr), _ptr(levels), _ptr(read_off),
                                               _ptr(level_val), _ptr(align_read), _ptr(flank), _ptr(flank_off),
                                               ctypes.c_int32(samples), _ptr(score), _ptr(j_end), _ptr(j0), _ptr(rec)))
        return score, j_end, j0, rec

    def last_timing(self):
        t = np.zeros(8, np.float32)
        self._check(self._lib.strq_last_timing(self._h, _ptr(t)))
        return t

    def last_counters(self):
        t = np.zeros(8, np.float64)
        self._check(self._lib.strq_last_counters(self._h, _ptr(t)))
        return t

    def last_viterbi_launches(self):
        """strq_last_viterbi_launches as a dict (flanked-model decode of the last sub-batch)."""
        g = np.zeros(4, np.int32)
        self._check(self._lib.strq_last_viterbi_launches(self._h, _ptr(g)))
        return dict(zip(("launches", "register_resident", "lane_layout", "general"), (int(v) for v in g)))

    def last_second_round(self):
        """strq_last_second_round: (alignments that ran the second forward round, alignments) of the last batched call."""
        g = np.zeros(2, np.int64)
        self._check(self._lib.strq_last_second_round(self._h, _ptr(g)))
        return int(g[0]), int(g[1])

    def last_screen(self):
        """strq_last_screen as a dict: what the upper-bound screen of the last batched call did."""
        g = np.zeros(8, np.float64)
        self._check(self._lib.strq_last_screen(self._h, _ptr(g)))
        keys = ("ms", "screened", "windowed", "whole_read", "window_columns", "wave_steps", "scale", "candidate_chunks")
        out = dict(zip(keys, (float(v) for v in g)))
        m = np.zeros(8, np.int32)
        self._check(self._lib.strq_last_screen_mode(self._h, _ptr(m)))
        out["mode"] = {0: None, 1: "fine", 2: "coarse"}.get(int(m[0]))
        out["coarse_pause"], out["fine_pause"], out["coarse_margin"], out["merge"] = int(m[1]), int(m[2]), int(m[3]), int(m[4])
        out["second_look"] = int(m[5])          # alignments resolved by the coarse screen's second look (not in strq_last_second_round)
        out["lds_layout"] = {0: None, 1: "lanes", 2: "rows", 3: "levels"}.get(int(m[6]))          # score tables of the two-flank screen kernels
        out["byte_scale"] = int(m[7])           # level image: the scale of the kernel's byte entries (its chunk values leave it at `scale`)
        return out

    def last_overlap(self):
        """strq_last_overlap as a dict: Viterbi ms harvested since the last run call started, and how much of it lay under the
        following sub-batch's screen kernel / whole alignment stage."""
        g = np.zeros(4, np.float64)
        self._check(self._lib.strq_last_overlap(self._h, _ptr(g)))
        return dict(zip(("viterbi_ms", "under_screen_ms", "under_alignment_stage_ms", "sub_batches"), (float(v) for v in g)))

    def last_geometry(self):
        """strq_last_geometry as a dict: which forward-DP kernel instance the last batched call ran."""
        g = np.zeros(8, np.int32)
        self._check(self._lib.strq_last_geometry(self._h, _ptr(g)))
        keys = ("waves_per_alignment", "tables_per_cu", "wpe", "rows_per_lane", "packed", "overlap_first", "overlap_worst", "launch_groups")
        return dict(zip(keys, (int(v) for v in g)))

    # ---- HMM ------------------------------------------------------------------------------
    def model_create(self, baked):
        mid = ctypes.c_int32(-1)
        arrs = [_c(baked.in_ptr, np.int32), _c(baked.in_src, np.int32), _c(baked.in_logp, np.float64),
                _c(baked.emis_kind, np.int32), _c(baked.emis_a, np.float64), _c(baked.emis_b, np.float64),
                _c(baked.emis_c, np.float64), _c(baked.count_inc, np.int32), _c(baked.tag, np.int32)]
        hints = getattr(baked, 'hint_slot', None) is not None and (np.asarray(baked.hint_slot)[:baked.silent_start] >= 0).all()
        arrs += [_c(baked.hint_slot, np.int32) if hints else None, _c(baked.hint_lane, np.int32) if hints else None]
        self._check(self._lib.strq_model_create(self._h, ctypes.c_int32(baked.n_states), ctypes.c_int32(baked.silent_start),
                                                ctypes.c_int32(baked.start), ctypes.c_int32(baked.end),
                                                *[_ptr(a) for a in arrs], ctypes.byref(mid)))
        self.__dict__.setdefault('_model_emit', {})[mid.value] = int(baked.silent_start)      # row length of viterbi_state_stats
        psum = getattr(baked, 'in_logp_sum', None)
        if psum is not None and len(psum) == len(baked.in_logp) and np.all(psum >= baked.in_logp) and not np.array_equal(psum, baked.in_logp):
            # edges that stand for several parallel paths: the forward pass sums them (the decode took the largest).  Arrays whose
            # in_logp was replaced after bake() carry a sum that no longer belongs to them: their in_logp stands alone
            self._check(self._lib.strq_model_set_forward_logp(self._h, mid, _ptr(_c(baked.in_logp_sum, np.float64))))
        self.last_positions_rc = self.last_positions_error = None
        if getattr(baked, 'pos_kind', None) is not None:
            # optional register-resident image (profile chains); a model that is no such chain keeps its lane layout
            rc = self._lib.strq_model_set_positions(self._h, mid, _ptr(_c(baked.pos_kind, np.int32)), _ptr(_c(baked.pos_index, np.int32)))
            self.last_positions_rc = rc
            # why the chain builder refused (a model that is no such chain keeps its lane layout): kept for whoever reports layouts
            self.last_positions_error = self._lib.strq_last_error(self._h).decode() if rc == STRQ_ERR_UNSUPPORTED else None
            if rc not in (STRQ_OK, STRQ_ERR_UNSUPPORTED):
                self._check(rc)
        return mid.value

    def viterbi_batch(self, model_id, seqs, want_path=False):
        """seqs: list of float64 arrays.  Returns (logp[], counted[], status[], paths or None)."""
        off = np.zeros(len(seqs) + 1, np.int64)
        for i, s in enumerate(seqs):
            off[i + 1] = off[i] + len(s)
        x = np.concatenate([_c(s, np.float64) for s in seqs]) if len(seqs) else np.zeros(0)
        n = len(seqs)
        logp = np.zeros(n); counted = np.zeros(n, np.int64); status = np.zeros(n, np.int32)
        paths = np.zeros(len(x), np.int32) if want_path else None
        self._check(self._lib.strq_viterbi_batch(self._h, ctypes.c_int32(model_id), ctypes.c_int64(n), _ptr(x), _ptr(off),
                                                 _ptr(logp), _ptr(counted), _ptr(status), _ptr(paths)))
        if want_path:
            paths = [paths[off[i]:off[i + 1]] for i in range(n)]
        return logp, counted, status, paths

    def debug_viterbi_mode(self, model_id, mode, seqs):
        """strq_debug_viterbi_mode: one Viterbi launch of decode mode `mode` (VIT_COUNT, VIT_MARK, VIT_HUB, VIT_UNIT) over the windows
        `seqs` (float64 arrays).  Returns a dict of raw results: 'logp', 'counted', 'status', 'dbg' (n, 4 uint32), 'records' (per
        window: hub T + 1 uint64, unit (T, 2) uint32, else None) and 'launched' (the shape id that ran)."""
        return self._debug_viterbi(model_id, mode, seqs, VIT_SRC_F64, None, False, False)

    def debug_viterbi_sourced(self, model_id, mode, kind, samples, consts, tracts=False):
        """strq_debug_viterbi_sourced: the same launch over windows given as the detect pipeline gives them -- `samples` a list of
        int16 (kind VIT_SRC_I16_AFFINE) or float64 (VIT_SRC_F64_AFFINE) arrays, `consts` one (c1, h1, h2, c2, lo, hi) per window.
        The dict of debug_viterbi_mode; with `tracts` (a count launch of a model with tracts) also 'tract_counts' (n, 3 int64)."""
        consts = _c(consts, np.float64).reshape(-1, 6)
        if len(consts) != len(samples):
            raise ValueError("consts must have one row per window")
        return self._debug_viterbi(model_id, mode, samples, kind, consts, tracts, True)

    def _debug_viterbi(self, model_id, mode, seqs, kind, consts, tracts, sourced):
        n = len(seqs)
        x, x_off = _offsets(seqs, np.int16 if kind == VIT_SRC_I16_AFFINE else np.float64)
        logp = np.zeros(n); counted = np.zeros(n, np.int64); status = np.zeros(n, np.int32); dbg = np.zeros((n, 4), np.uint32)
        launched = np.full(1, -1, np.int32)
        rec = rec_off = None
        if mode in (VIT_HUB, VIT_UNIT):
            rec_off = np.zeros(n + 1, np.int64)
            for i, s in enumerate(seqs):
                rec_off[i + 1] = rec_off[i] + (8 * (len(s) + 1) if mode == VIT_HUB else 8 * len(s))
            rec = np.full(int(rec_off[-1]) + 8, 0xA5, np.uint8)
        tcounts = np.zeros((n, 3), np.int64) if tracts else None
        if not sourced:
            self._check(self._lib.strq_debug_viterbi_mode(self._h, ctypes.c_int32(model_id), ctypes.c_int32(mode), ctypes.c_int64(n), _ptr(x), _ptr(x_off),
                                                          _ptr(logp), _ptr(counted), _ptr(status), _ptr(dbg), _ptr(rec), _ptr(rec_off), _ptr(launched)))
        else:
            self._check(self._lib.strq_debug_viterbi_sourced(self._h, ctypes.c_int32(model_id), ctypes.c_int32(mode), ctypes.c_int32(kind),
                                                             ctypes.c_int32(1 if tracts else 0), ctypes.c_int64(n), _ptr(x), _ptr(x_off), _ptr(consts),
                                                             _ptr(logp), _ptr(counted), _ptr(status), _ptr(dbg), _ptr(rec), _ptr(rec_off), _ptr(tcounts),
                                                             _ptr(launched)))
        records = [None] * n
        if rec is not None:
            for i in range(n):
                raw = rec[int(rec_off[i]):int(rec_off[i + 1])]
                records[i] = raw.view(np.uint64).copy() if mode == VIT_HUB else raw.view(np.uint32).reshape(-1, 2).copy()
        out = {"logp": logp, "counted": counted, "status": status, "dbg": dbg, "records": records, "launched": int(launched[0])}
        if tracts:
            out["tract_counts"] = tcounts
        return out

    def forward_batch(self, model_id, xs, c0=None):
        """strq_forward_batch: xs a list of float64 arrays; c0 None or one int per window (the moments are accumulated about it:
        pass the Viterbi visit count).  Returns (log_lik[], visits_mean[], visits_var[], status[])."""
        n = len(xs)
        off = np.zeros(n + 1, np.int64)
        for i, s in enumerate(xs):
            off[i + 1] = off[i] + len(s)
        x = np.concatenate([_c(s, np.float64) for s in xs]) if n else np.zeros(0)
        if len(x) == 0:
            x = np.zeros(1)
        ll = np.zeros(n); mean = np.zeros(n); var = np.zeros(n); status = np.zeros(n, np.int32)
        c0a = None if c0 is None else _c(c0, np.int64)
        if c0a is not None and len(c0a) != n:
            raise ValueError("c0 must have one entry per window")
        self._check(self._lib.strq_forward_batch(self._h, ctypes.c_int32(model_id), ctypes.c_int64(n), _ptr(x), _ptr(off), _ptr(c0a),
                                                 _ptr(ll), _ptr(mean), _ptr(var), _ptr(status)))
        return ll, mean, var, status

    def model_set_tracts(self, model_id, n_tracts, tract_of):
        """strq_model_set_tracts: tract_of one entry per state, -1 or the tract (0 .. n_tracts - 1) whose counter an emission of
        the state advances."""
        self._check(self._lib.strq_model_set_tracts(self._h, ctypes.c_int32(model_id), ctypes.c_int32(n_tracts), _ptr(_c(tract_of, np.int32))))

    def viterbi_tracts(self, model_id, xs):
        """strq_viterbi_tracts: xs a list of float64 arrays.  Returns (logp[], counts (n, 3) int64, status[]); status 0 ok, 1 no
        path, 2 a window of 2^21 observations or more (not decoded)."""
        n = len(xs)
        x, off = _offsets(xs, np.float64)
        logp = np.zeros(n); counts = np.zeros((n, 3), np.int64); status = np.zeros(n, np.int32)
        self._check(self._lib.strq_viterbi_tracts(self._h, ctypes.c_int32(model_id), ctypes.c_int64(n), _ptr(x), _ptr(off),
                                                  _ptr(logp), _ptr(counts), _ptr(status)))
        return logp, counts, status

    def viterbi_tract_positions(self, model_id, xs):
        """strq_viterbi_tract_positions: viterbi_tracts plus the positions.  Returns (logp[], counts (n, 3) int64, status[],
        positions): positions[i] a tuple of three ascending np.int64 arrays of observation indices, tract by tract in model order
        (empty beyond the model's tracts, without a path, and for status 4: the window's back-pointers exceed
        STRQ_TRACT_POS_WS_BYTES -- counts valid, not traced)."""
        n = len(xs)
        x, off = _offsets(xs, np.float64)
        logp = np.zeros(n); counts = np.zeros((n, 3), np.int64); status = np.zeros(max(1, n), np.int32)
        pos_off = np.zeros(3 * n + 1, np.int64); pool = np.zeros(max(1, int(off[-1])), np.int64)      # (a tract emits each observation at most once)
        self._check(self._lib.strq_viterbi_tract_positions(self._h, ctypes.c_int32(model_id), ctypes.c_int64(n), _ptr(x), _ptr(off), _ptr(logp), _ptr(counts),
                                                           _ptr(status), _ptr(pos_off), _ptr(pool), ctypes.c_int64(len(pool))))
        return logp, counts, status[:n], [tuple(pool[pos_off[3 * i + j]:pos_off[3 * i + j + 1]].copy() for j in range(3)) for i in range(n)]

    def viterbi_state_stats(self, model_id, xs):
        """strq_viterbi_state_stats: xs a list of float64 arrays (NaN: missing).  Returns (logp[], counted[], status[], n, sum,
        sumsq): logp / counted as viterbi_batch gives them, n (int64), sum and sumsq (float64) of shape (windows, silent_start) --
        what the best path assigns to every emitting state (strique_amd/state_stats.py); status 0 ok, 1 no path, 4 the window's
        back-pointers exceed STRQ_STATE_STATS_WS_BYTES (logp and counted valid, zero rows)."""
        n = len(xs)
        x, off = _offsets(xs, np.float64)
        n_emit = int(self._model_emit[model_id])
        logp = np.zeros(n); counted = np.zeros(n, np.int64); status = np.zeros(max(1, n), np.int32)
        cnt = np.zeros((max(1, n), n_emit), np.int64); s1 = np.zeros((max(1, n), n_emit)); s2 = np.zeros((max(1, n), n_emit))
        self._check(self._lib.strq_viterbi_state_stats(self._h, ctypes.c_int32(model_id), ctypes.c_int64(n), _ptr(x), _ptr(off), _ptr(logp), _ptr(counted),
                                                       _ptr(status), _ptr(cnt), _ptr(s1), _ptr(s2)))
        return logp, counted, status[:n], cnt[:n], s1[:n], s2[:n]

    def forward_state_stats(self, model_id, xs):
        """strq_forward_state_stats: xs a list of float64 arrays (NaN: missing).  Returns (log_lik[], status[], w, wx, wxx): w, wx
        and wxx (float64) of shape (windows, silent_start) -- per emitting state the posterior occupancy over all paths and its
        first two moments of the observations (strique_amd/state_posteriors.py); status 0 ok, 1 no path (zero rows, log_lik -inf),
        4 the window's stored forward vectors exceed STRQ_STATE_POST_WS_BYTES (log_lik valid, zero rows)."""
        n = len(xs)
        x, off = _offsets(xs, np.float64)
        n_emit = int(self._model_emit[model_id])
        ll = np.zeros(max(1, n)); status = np.zeros(max(1, n), np.int32)
        w = np.zeros((max(1, n), n_emit)); wx = np.zeros((max(1, n), n_emit)); wxx = np.zeros((max(1, n), n_emit))
        self._check(self._lib.strq_forward_state_stats(self._h, ctypes.c_int32(model_id), ctypes.c_int64(n), _ptr(x), _ptr(off), _ptr(ll), _ptr(status),
                                                       _ptr(w), _ptr(wx), _ptr(wxx)))
        return ll[:n], status[:n], w[:n], wx[:n], wxx[:n]

    def motif_track(self, model_ids, xs, segment=256):
        """strq_motif_track: model_ids the loop models of the K = 2 to 4 candidates (motifs.loop_arrays through model_create), xs a
        list of float64 arrays of at least one observation (NaN: missing).  Returns per window (V (n_seg, K) float64, winners
        (n_seg,) int32, obs_won (K,) int64, majority): strique_amd/motifs.py states the rule."""
        n, K = len(xs), len(model_ids)
        if any(len(s) < 1 for s in xs):
            raise ValueError("motif_track: a window needs at least one observation")
        x, off = _offsets(xs, np.float64)
        cap = sum(max(1, len(s) // max(1, int(segment))) for s in xs)
        V = np.zeros((max(1, cap), max(1, K))); win = np.zeros(max(1, cap), np.int32)
        n_seg = np.zeros(max(1, n), np.int64); won = np.zeros((max(1, n), 4), np.int64); maj = np.zeros(max(1, n), np.int32)
        self._check(self._lib.strq_motif_track(self._h, ctypes.c_int32(K), _ptr(_c(model_ids, np.int32)), ctypes.c_int32(segment), ctypes.c_int64(n),
                                               _ptr(x), _ptr(off), ctypes.c_int64(cap), _ptr(V), _ptr(win), _ptr(n_seg), _ptr(won), _ptr(maj)))
        out, at = [], 0
        for i in range(n):
            k = int(n_seg[i])
            out.append((V[at:at + k].copy(), win[at:at + k].copy(), won[i, :K].copy(), int(maj[i])))
            at += k
        return out

    def debug_tract_shape(self):
        """strq_debug_tract_shape: the kernel shape id of this context's last tract launch (-1: none yet)."""
        shape = ctypes.c_int32(-1)
        self._check(self._lib.strq_debug_tract_shape(self._h, ctypes.byref(shape)))
        return int(shape.value)

    def viterbi(self, model_id, x, want_path=True):
        logp, counted, status, paths = self.viterbi_batch(model_id, [x], want_path)
        return logp[0], int(counted[0]), int(status[0]), (paths[0] if want_path else None)

    # ---- detect pipeline ------------------------------------------------------------------
    def set_pore_stats(self, tail_lo, tail_hi, model_min, model_max):
        self._check(self._lib.strq_set_pore_stats(self._h, ctypes.c_double(tail_lo), ctypes.c_double(tail_hi),
                                                  ctypes.c_double(model_min), ctypes.c_double(model_max)))

    def target_add(self, prefix_ext, suffix_ext, trim_prefix, trim_suffix, samples, model_id, count_bias):
        pe = _c(prefix_ext, np.float32); se = _c(suffix_ext, np.float32)
        tid = ctypes.c_int32(-1)
        self._check(self._lib.strq_target_add(self._h, _ptr(pe), ctypes.c_int64(len(pe)), _ptr(se), ctypes.c_int64(len(se)),
                                              ctypes.c_int32(trim_prefix), ctypes.c_int32(trim_suffix), ctypes.c_int32(samples),
                                              ctypes.c_int32(model_id), ctypes.c_int32(count_bias), ctypes.byref(tid)))
        return tid.value

    def target_set_mod(self, target_id, mod_model_id, mod_min, mod_max):
        self._check(self._lib.strq_target_set_mod(self._h, ctypes.c_int32(target_id), ctypes.c_int32(mod_model_id),
                                                  ctypes.c_double(mod_min), ctypes.c_double(mod_max)))

    def batch_fetch_mod(self):
        off = np.zeros(self._n_batch + 1, np.int64)
        self._check(self._lib.strq_batch_fetch_mod(self._h, None, ctypes.c_int64(0), _ptr(off)))
        pool = np.zeros(max(1, int(off[-1])), np.uint8)
        self._check(self._lib.strq_batch_fetch_mod(self._h, _ptr(pool), ctypes.c_int64(len(pool)), _ptr(off)))
        raw = pool.tobytes()
        return [raw[off[i]:off[i + 1]].decode() for i in range(self._n_batch)]

    def _last(self, entry, keys, floats=("ms",)):
        """strq_last_<entry> as a dict: `keys` in the order of the entry's layout, integers but for `floats`."""
        out = np.zeros(len(keys))
        self._check(getattr(self._lib, "strq_last_" + entry)(self._h, _ptr(out)))
        return {k: float(v) if k in floats else int(v) for k, v in zip(keys, out)}

    def _fetch_records(self, entry, dtype):
        """strq_batch_fetch_<entry>: one element of `dtype` per read of the last batch."""
        n = getattr(self, '_n_batch', 0)
        out = np.zeros(max(1, n), dtype=dtype)
        self._check(getattr(self._lib, "strq_batch_fetch_" + entry)(self._h, _ptr(out), ctypes.c_int64(n)))
        return out[:n]

    def _switch(self, entry, on, level=None):
        """strq_set_<entry>: the pass on or off; `level` for an entry that takes one with it (0.0 when switching off)."""
        args = [ctypes.c_int32(1 if on else 0)] + ([] if level is None else [ctypes.c_double(level if on else 0.0)])
        self._check(getattr(self._lib, "strq_set_" + entry)(self._h, *args))

    def set_units(self, on):
        """strq_set_units: later run calls also produce repeat-unit positions (batch_fetch_units)."""
        self._switch("units", on)

    def batch_fetch_units(self):
        """Unit positions of the last batch: one ascending np.int64 array of raw-signal sample indices per read, or None for a
        read that was not decoded (strq_batch_fetch_units)."""
        n = getattr(self, '_n_batch', 0)
        off = np.zeros(n + 1, np.int64); dec = np.zeros(max(1, n), np.int32)
        self._check(self._lib.strq_batch_fetch_units(self._h, None, ctypes.c_int64(0), _ptr(off), _ptr(dec)))
        pool = np.zeros(max(1, int(off[-1])), np.int64)
        self._check(self._lib.strq_batch_fetch_units(self._h, _ptr(pool), ctypes.c_int64(len(pool)), _ptr(off), _ptr(dec)))
        return [pool[off[i]:off[i + 1]].copy() if dec[i] else None for i in range(n)]

    def last_units(self):
        """The unit pass of the last run call: {'ms', 'ws_bytes', 'windows', 'positions'} (strq_last_units)."""
        return self._last("units", ("ms", "ws_bytes", "windows", "positions"), floats=("ms", "ws_bytes"))

    def set_confidence(self, on):
        """strq_set_confidence: later run calls also run the forward pass over every decoded window (batch_fetch_confidence)."""
        self._switch("confidence", on)

    def batch_fetch_confidence(self):
        """Confidence of the last batch: per read (log_lik, count_mean, count_sd) as Python floats, or None for a read that was
        not decoded (strq_batch_fetch_confidence)."""
        n = getattr(self, '_n_batch', 0)
        out = np.zeros((max(1, n), 3), np.float64); dec = np.zeros(max(1, n), np.int32)
        self._check(self._lib.strq_batch_fetch_confidence(self._h, _ptr(out), _ptr(dec)))
        return [(float(out[i, 0]), float(out[i, 1]), float(out[i, 2])) if dec[i] else None for i in range(n)]

    def last_confidence(self):
        """The forward pass of the last run call: {'ms', 'windows', 'no_path', 'max_exponent'} (strq_last_confidence)."""
        return self._last("confidence", ("ms", "windows", "no_path", "max_exponent"))

    def set_mod_llr(self, on):
        """strq_set_mod_llr: later run calls also score every repeat unit of a modification pattern under both branches of the
        dual model (batch_fetch_mod_llr).  StriqueHipError (STRQ_ERR_UNSUPPORTED) for a modification model the pass does not cover."""
        self._switch("mod_llr", on)

    def batch_fetch_mod_llr(self):
        """Per-unit scores of the last batch: per read an (n_units, 2) float64 array of (V_base, V_mod), one row per character of
        its modification pattern, or None for a read without units (strq_batch_fetch_mod_llr)."""
        n = getattr(self, '_n_batch', 0)
        off = np.zeros(n + 1, np.int64)
        self._check(self._lib.strq_batch_fetch_mod_llr(self._h, None, ctypes.c_int64(0), _ptr(off)))
        pool = np.zeros((max(1, int(off[-1])), 2), np.float64)
        self._check(self._lib.strq_batch_fetch_mod_llr(self._h, _ptr(pool), ctypes.c_int64(len(pool)), _ptr(off)))
        return [pool[off[i]:off[i + 1]].copy() if off[i + 1] > off[i] else None for i in range(n)]

    def last_mod_llr(self):
        """The scoring pass of the last run call: {'ms', 'units', 'reads', 'launches'} (strq_last_mod_llr)."""
        return self._last("mod_llr", ("ms", "units", "reads", "launches"))

    # ---- variants ------------------------------------------------------------------------
    def target_set_variants(self, target_id, model_id, lo, hi, n_alt, context_units):
        """strq_target_set_variants: the variant model of a target (hmm.RepeatVariantModel), the range its stretch is clipped to, its
        alt branches and context units; model_id = -1 takes it away.  StriqueHipError (STRQ_ERR_UNSUPPORTED) for a model the pass
        does not cover: the target stays as it was."""
        self._check(self._lib.strq_target_set_variants(self._h, ctypes.c_int32(target_id), ctypes.c_int32(model_id), ctypes.c_double(lo), ctypes.c_double(hi),
                                                       ctypes.c_int32(n_alt), ctypes.c_int32(context_units)))

    def set_variants(self, on):
        """strq_set_variants: later run calls also decode the variant model of every decoded read whose target has one
        (batch_fetch_variants)."""
        self._switch("variants", on)

    def batch_fetch_variants(self):
        """Variants of the last batch (strq_batch_fetch_variants): per read None (not decoded, or a target without a variant model) or
        (count_v, branch int8 [n], end int64 [n], V float64 [n, n_branches]) of its n passages in signal order."""
        n = getattr(self, '_n_batch', 0)
        count_v = np.zeros(max(1, n), np.int32); dec = np.zeros(max(1, n), np.int32); off = np.zeros(n + 1, np.int64)
        vt = ctypes.c_int64(0)
        self._check(self._lib.strq_batch_fetch_variants(self._h, _ptr(count_v), _ptr(dec), _ptr(off), None, None, ctypes.c_int64(0),
                                                        None, None, ctypes.c_int64(0), ctypes.byref(vt)))
        npass = int(off[-1])
        branch = np.zeros(max(1, npass), np.int8); end = np.zeros(max(1, npass), np.int64)
        vpool = np.zeros(max(1, vt.value), np.float64); voff = np.zeros(npass + 1, np.int64)
        self._check(self._lib.strq_batch_fetch_variants(self._h, _ptr(count_v), _ptr(dec), _ptr(off), _ptr(branch), _ptr(end), ctypes.c_int64(len(branch)),
                                                        _ptr(vpool), _ptr(voff), ctypes.c_int64(len(vpool)), None))
        out = []
        for i in range(n):
            if not dec[i]:
                out.append(None)
                continue
            a, b = int(off[i]), int(off[i + 1])
            nb = int(voff[a + 1] - voff[a]) if b > a else 0
            V = vpool[voff[a]:voff[b]].reshape(b - a, nb).copy() if b > a else np.zeros((0, 0))
            out.append((int(count_v[i]), branch[a:b].copy(), end[a:b].copy(), V))
        return out

    def last_variants(self):
        """The variant pass of the last run call: {'launches', 'passages', 'ms', 'reads'} (strq_last_variants)."""
        return self._last("variants", ("launches", "passages", "ms", "reads"))

    # ---- anchored counting ---------------------------------------------------------------
    def target_set_anchored(self, target_id, end_model_id, end_bias, start_model_id, start_bias):
        """strq_target_set_anchored: the end / start model of a target (hmm.AnchoredRepeatModel) and their count biases."""
        self._check(self._lib.strq_target_set_anchored(self._h, ctypes.c_int32(target_id), ctypes.c_int32(end_model_id), ctypes.c_int32(end_bias),
                                                       ctypes.c_int32(start_model_id), ctypes.c_int32(start_bias)))

    def set_anchored(self, on, min_score=0.0):
        """strq_set_anchored: later run calls also classify every read (strique_amd.anchored) and decode those that hold one flank
        only.  StriqueHipError (STRQ_ERR_ARG) for a min_score that is not above 0."""
        self._switch("anchored", on, min_score)

    def batch_fetch_anchored(self):
        """Records of the last batch (strq_batch_fetch_anchored): a structured array of ANCHORED_DTYPE, one element per read."""
        return self._fetch_records("anchored", ANCHORED_DTYPE)

    def last_anchored(self):
        """The anchored pass of the last run call (strq_last_anchored): {'ms', 'kinds' (reads of kind 0..3), 'launches',
        'register_resident', 'lane_layout' (windows decoded on those kernel shapes)}."""
        d = self._last("anchored", ("ms", 0, 1, 2, 3, "launches", "register_resident", "lane_layout"))
        return {'ms': d['ms'], 'kinds': tuple(d[k] for k in range(4)), **{k: d[k] for k in ('launches', 'register_resident', 'lane_layout')}}

    def target_set_tracts(self, target_id, model_id, n_tracts=0, bias=()):
        """strq_target_set_tracts: the compound model of a target (hmm.CompoundRepeatModel, with model_set_tracts applied) and the
        count bias of each of its tracts; model_id -1 takes it away."""
        b = np.zeros(3, np.int32)
        b[:len(bias)] = bias
        self._check(self._lib.strq_target_set_tracts(self._h, ctypes.c_int32(target_id), ctypes.c_int32(model_id), ctypes.c_int32(n_tracts), _ptr(b)))

    def set_tracts(self, on):
        """strq_set_tracts: later run calls also decode the compound model of every decoded read whose target has one
        (batch_fetch_tracts)."""
        self._switch("tracts", on)

    def batch_fetch_tracts(self):
        """Records of the last batch (strq_batch_fetch_tracts): a structured array of TRACTS_DTYPE, one element per read."""
        return self._fetch_records("tracts", TRACTS_DTYPE)

    def last_tracts(self):
        """The tract pass of the last run call (strq_last_tracts): {'ms', 'windows' (decoded), 'launches', 'failed' (status 2 or 3)}."""
        return self._last("tracts", ("ms", "windows", "launches", "failed"))

    def target_set_motifs(self, target_id, loop_model_ids=(), flanked_model_ids=(), bias=()):
        """strq_target_set_motifs: the candidates of a target -- per candidate its loop model (motifs.loop_arrays), the flanked model
        of that unit and its count bias; candidate 0 is the unit of the target's own model (its flanked id is not read).  No ids:
        the candidates are taken away."""
        n = len(loop_model_ids)
        if len(flanked_model_ids) != n or len(bias) != n:
            raise ValueError("target_set_motifs: one loop model, one flanked model and one bias per candidate")
        a, b, c = (np.zeros(4, np.int32) for _ in range(3))
        a[:n] = loop_model_ids; b[:n] = flanked_model_ids; c[:n] = bias
        self._check(self._lib.strq_target_set_motifs(self._h, ctypes.c_int32(target_id), ctypes.c_int32(n), _ptr(a), _ptr(b), _ptr(c)))

    def set_motifs(self, on, segment=256):
        """strq_set_motifs: later run calls also score the stretch between the flanks of every read whose target has candidates,
        in segments of `segment` observations (batch_fetch_motifs; strique_amd/motifs.py states the rule)."""
        self._check(self._lib.strq_set_motifs(self._h, ctypes.c_int32(1 if on else 0), ctypes.c_int32(segment if on else 0)))

    def batch_fetch_motifs(self):
        """The motif track of the last batch (strq_batch_fetch_motifs): (records, V, winners) -- a structured array of MOTIFS_DTYPE
        with one element per read, and per read the scores (n_seg, n_cand) float64 and the winners (n_seg,) int32 (empty for a read
        that was not scored)."""
        n = getattr(self, '_n_batch', 0)
        rec = np.zeros(max(1, n), dtype=MOTIFS_DTYPE); off = np.zeros(n + 1, np.int64)
        self._check(self._lib.strq_batch_fetch_motifs(self._h, _ptr(rec), ctypes.c_int64(n), _ptr(off), None, None, ctypes.c_int64(0)))
        m = max(1, int(off[-1]))
        V = np.zeros((m, 4)); win = np.zeros(m, np.int32)
        self._check(self._lib.strq_batch_fetch_motifs(self._h, _ptr(rec), ctypes.c_int64(n), _ptr(off), _ptr(V), _ptr(win), ctypes.c_int64(m)))
        rec = rec[:n]
        return (rec, [V[off[i]:off[i + 1], :int(rec[i]['n_cand'])].copy() for i in range(n)], [win[off[i]:off[i + 1]].copy() for i in range(n)])

    def last_motifs(self):
        """The motif pass of the last run call (strq_last_motifs): {'ms', 'reads' (scored), 'segments', 'launches', 'decodes' (of
        reads whose majority is not the configured unit)}."""
        return self._last("motifs", ("ms", "reads", "segments", "launches", "decodes"))

    def set_tract_positions(self, on):
        """strq_set_tract_positions: later run calls with set_tracts on also trace every tract window of status 0 back
        (batch_fetch_tract_positions)."""
        self._switch("tract_positions", on)

    def batch_fetch_tract_positions(self):
        """Tract positions of the last batch (strq_batch_fetch_tract_positions): per read (pos_status, positions) -- pos_status 0
        and a tuple of three ascending np.int64 arrays of raw-signal sample indices in model order (empty beyond the model's
        tracts), or 1 (the tract record's status is not 0) / 2 (back-pointers over the budget) and None."""
        n = getattr(self, '_n_batch', 0)
        off = np.zeros(3 * n + 1, np.int64); ps = np.zeros(max(1, n), np.int32)
        self._check(self._lib.strq_batch_fetch_tract_positions(self._h, _ptr(ps), _ptr(off), None, ctypes.c_int64(0)))
        pool = np.zeros(max(1, int(off[-1])), np.int64)
        self._check(self._lib.strq_batch_fetch_tract_positions(self._h, _ptr(ps), _ptr(off), _ptr(pool), ctypes.c_int64(len(pool))))
        return [(int(ps[i]), tuple(pool[off[3 * i + j]:off[3 * i + j + 1]].copy() for j in range(3)) if ps[i] == 0 else None) for i in range(n)]

    def last_tract_positions(self):
        """The tract-position pass of the last run call (strq_last_tract_positions): {'ms', 'windows' (traced), 'launches', 'bp_bytes'
        (peak back-pointer bytes of a piece)}."""
        return self._last("tract_positions", ("ms", "windows", "launches", "bp_bytes"), floats=("ms", "bp_bytes"))

    def set_state_stats(self, on):
        """strq_set_state_stats: later run calls also sum, per emitting state of the flanked model, the observations the best path
        assigns to it (batch_fetch_state_stats; strique_amd/state_stats.py states the rule)."""
        self._switch("state_stats", on)

    def batch_fetch_state_stats(self, with_status=False):
        """State statistics of the last batch (strq_batch_fetch_state_stats): per read None, or (n, sum, sumsq) -- np.int64 / float64
        arrays with one entry per emitting state of the read's flanked model.  with_status: (status[], that list) -- 0 statistics,
        1 none, 2 back-pointers over the budget."""
        n = getattr(self, '_n_batch', 0)
        off = np.zeros(n + 1, np.int64); st = np.zeros(max(1, n), np.int32)
        self._check(self._lib.strq_batch_fetch_state_stats(self._h, _ptr(off), None, None, None, ctypes.c_int64(0), _ptr(st)))
        m = max(1, int(off[-1]))
        cnt = np.zeros(m, np.int64); s1 = np.zeros(m); s2 = np.zeros(m)
        self._check(self._lib.strq_batch_fetch_state_stats(self._h, _ptr(off), _ptr(cnt), _ptr(s1), _ptr(s2), ctypes.c_int64(m), _ptr(st)))
        out = [None if st[i] != 0 else (cnt[off[i]:off[i + 1]].copy(), s1[off[i]:off[i + 1]].copy(), s2[off[i]:off[i + 1]].copy()) for i in range(n)]
        return (st[:n].copy(), out) if with_status else out

    def last_state_stats(self):
        """The state-statistics pass of the last run call (strq_last_state_stats): {'ms', 'windows' (traced), 'launches', 'bp_bytes'
        (peak back-pointer bytes of a piece)}."""
        return self._last("state_stats", ("ms", "windows", "launches", "bp_bytes"), floats=("ms", "bp_bytes"))

    def set_state_posteriors(self, on):
        """strq_set_state_posteriors: later run calls also run forward-backward over every decoded window and sum, per emitting state
        of the flanked model, its posterior occupancy (batch_fetch_state_posteriors; strique_amd/state_posteriors.py states the rule)."""
        self._switch("state_posteriors", on)

    def batch_fetch_state_posteriors(self, with_status=False):
        """State posteriors of the last batch (strq_batch_fetch_state_posteriors): per read None, or (w, wx, wxx, log_lik) -- float64
        arrays with one entry per emitting state of the read's flanked model and the forward log-likelihood of its window.
        with_status: (status[], that list) -- 0 statistics, 1 none, 2 stored vectors over the budget."""
        n = getattr(self, '_n_batch', 0)
        off = np.zeros(n + 1, np.int64); st = np.zeros(max(1, n), np.int32); ll = np.zeros(max(1, n))
        self._check(self._lib.strq_batch_fetch_state_posteriors(self._h, _ptr(off), None, None, None, ctypes.c_int64(0), _ptr(ll), _ptr(st)))
        m = max(1, int(off[-1]))
        w = np.zeros(m); wx = np.zeros(m); wxx = np.zeros(m)
        self._check(self._lib.strq_batch_fetch_state_posteriors(self._h, _ptr(off), _ptr(w), _ptr(wx), _ptr(wxx), ctypes.c_int64(m), _ptr(ll), _ptr(st)))
        out = [None if st[i] != 0 else (w[off[i]:off[i + 1]].copy(), wx[off[i]:off[i + 1]].copy(), wxx[off[i]:off[i + 1]].copy(), float(ll[i])) for i in range(n)]
        return (st[:n].copy(), out) if with_status else out

    def last_state_posteriors(self):
        """The state-posteriors pass of the last run call (strq_last_state_posteriors): {'ms', 'windows', 'launches', 'ws_bytes' (peak
        bytes of stored forward vectors of a piece)}."""
        return self._last("state_posteriors", ("ms", "windows", "launches", "ws_bytes"), floats=("ms", "ws_bytes"))

    def target_set_flank_mod(self, target_id, which, profile_model_id, flank_len, column_of, groups):
        """strq_target_set_flank_mod: the models of flank `which` (0 prefix, 1 suffix, as the strand of the target reads it) --
        column_of one entry per emitting state of the profile model, groups rows of (c0, c1, site model id, flank as configured, pos,
        n_sites)."""
        col = _c(column_of, np.int32)
        g = _c(groups if len(groups) else np.zeros((0, 6)), np.int32).reshape(-1, 6)
        self._check(self._lib.strq_target_set_flank_mod(self._h, ctypes.c_int32(target_id), ctypes.c_int32(which), ctypes.c_int32(profile_model_id),
                                                        ctypes.c_int32(flank_len), _ptr(col), ctypes.c_int32(len(g)), _ptr(g) if len(g) else None))

    def set_flank_mod(self, on):
        """strq_set_flank_mod: later run calls also call the CpG groups of the flanks (batch_fetch_flank_mod)."""
        self._switch("flank_mod", on)

    def batch_fetch_flank_mod(self):
        """Flank methylation calls of the last batch (strq_batch_fetch_flank_mod): per read None (it did not qualify) or a structured
        array of FLANK_MOD_DTYPE, one element per group of a flank whose stretch exists, prefix groups first."""
        n = getattr(self, '_n_batch', 0)
        called = np.zeros(max(1, n), np.int32); off = np.zeros(n + 1, np.int64)
        self._check(self._lib.strq_batch_fetch_flank_mod(self._h, _ptr(called), _ptr(off), None, ctypes.c_int64(0)))
        pool = np.zeros(max(1, int(off[-1])), FLANK_MOD_DTYPE)
        self._check(self._lib.strq_batch_fetch_flank_mod(self._h, _ptr(called), _ptr(off), _ptr(pool), ctypes.c_int64(len(pool))))
        return [pool[int(off[i]):int(off[i + 1])].copy() if called[i] else None for i in range(n)]

    def last_flank_mod(self):
        """The flank-mod pass of the last run call (strq_last_flank_mod): {'ms', 'flanks' (decoded), 'groups' (scored), 'launches'}."""
        return self._last("flank_mod", ("ms", "flanks", "groups", "launches"))

    def set_anchored_mod(self, on):
        """strq_set_anchored_mod: later run calls with anchored counting on also call the methylation pattern of every read of
        kind 2 / 3 whose record was decoded and whose target has a modification model (batch_fetch_anchored_mod)."""
        self._switch("anchored_mod", on)

    def batch_fetch_anchored_mod(self):
        """Methylation calls of the anchored reads of the last batch (strq_batch_fetch_anchored_mod): per read None (no call), or
        (pattern, scores) -- the pattern string ('-' when the dual model found no path) and an (n_units, 2) float64 array of
        (V_base, V_mod), one row per character, or None when the run call ran without set_mod_llr or the pattern has no units."""
        n = getattr(self, '_n_batch', 0)
        called = np.zeros(max(1, n), np.int32); off = np.zeros(n + 1, np.int64); voff = np.zeros(n + 1, np.int64)
        self._check(self._lib.strq_batch_fetch_anchored_mod(self._h, _ptr(called), _ptr(off), None, ctypes.c_int64(0), _ptr(voff), None, ctypes.c_int64(0)))
        chars = np.zeros(max(1, int(off[-1])), np.uint8); pool = np.zeros((max(1, int(voff[-1])), 2), np.float64)
        self._check(self._lib.strq_batch_fetch_anchored_mod(self._h, _ptr(called), _ptr(off), _ptr(chars), ctypes.c_int64(len(chars)), _ptr(voff), _ptr(pool),
                                                            ctypes.c_int64(len(pool))))
        out = []
        for i in range(n):
            if not called[i]:
                out.append(None)
                continue
            out.append((chars[off[i]:off[i + 1]].tobytes().decode('ascii'), pool[voff[i]:voff[i + 1]].copy() if voff[i + 1] > voff[i] else None))
        return out

    def last_anchored_mod(self):
        """The methylation calls of the last run call (strq_last_anchored_mod): {'ms', 'reads', 'units', 'launches'}."""
        return self._last("anchored_mod", ("ms", "reads", "units", "launches"))

    # ---- renorm: the second normalisation step ---------------------------------------------
    def target_set_renorm(self, target_id, Q, A, model_min, model_max):
        """strq_target_set_renorm: the tables of a target (strique_amd.renorm.tables) with the rule's shares and its grid over
        [model_min, model_max]."""
        from . import renorm
        Q = _c(Q, np.int16); A = _c(A, np.int32); W = _c(renorm.W, np.float64)
        if Q.shape != (renorm.N_W, renorm.GRID) or A.shape != (renorm.A_MAX + 1,):
            raise ValueError("renorm tables: Q[%d][%d], A[%d]" % (renorm.N_W, renorm.GRID, renorm.A_MAX + 1))
        lo, d, p = renorm.grid(model_min, model_max)
        self._check(self._lib.strq_target_set_renorm(self._h, ctypes.c_int32(target_id), _ptr(Q), ctypes.c_int32(renorm.Q_OUT), _ptr(A), _ptr(W),
                                                     ctypes.c_double(lo), ctypes.c_double(d), ctypes.c_double(p)))

    def set_renorm(self, on, min_share=0.0):
        """strq_set_renorm: later run calls refit the maps of every read against its target's composition and fold the fit in where
        the fitted repeat share reaches min_share.  StriqueHipError (STRQ_ERR_ARG) for a min_share outside (0, 1), or with a scan set."""
        self._switch("renorm", on, min_share)

    def batch_fetch_renorm(self):
        """Records of the last batch (strq_batch_fetch_renorm): a structured array of RENORM_DTYPE, one element per read; 'fit' holds
        the morphology levels, the filtered and the raw signal in that order."""
        return self._fetch_records("renorm", RENORM_DTYPE)

    def debug_renorm_fit(self, target_id, h3):
        """strq_debug_renorm_fit: the fit kernel alone on three histograms (uint32 [3, 1024]); one element of RENORM_DTYPE."""
        h3 = _c(h3, np.uint32)
        if h3.shape != (3, 1024):
            raise ValueError("three histograms of 1024 counters")
        out = np.zeros(1, dtype=RENORM_DTYPE)
        self._check(self._lib.strq_debug_renorm_fit(self._h, ctypes.c_int32(target_id), _ptr(h3), _ptr(out)))
        return out[0]

    def last_renorm(self):
        """The renorm pass of the last run call (strq_last_renorm): {'ms', 'fitted', 'applied', 'launches'}."""
        return self._last("renorm", ("ms", "fitted", "applied", "launches"))

    def batch_upload(self, signals, offsets, target_ids, host_stats=None):
        """signals: one concatenated int16 or float64 array; offsets: n_reads + 1."""
        signals = np.ascontiguousarray(signals)
        if signals.dtype == np.int16:
            dtype = 0
        elif signals.dtype == np.float64:
            dtype = 1
        else:
            raise ValueError("signals must be int16 or float64")
        offsets = _c(offsets, np.int64); target_ids = _c(target_ids, np.int32)
        hs = None if host_stats is None else _c(host_stats, np.float64)
        self._n_batch = len(target_ids)
        self._check(self._lib.strq_batch_upload(self._h, ctypes.c_int64(len(target_ids)), _ptr(signals), ctypes.c_int32(dtype),
                                                _ptr(offsets), _ptr(target_ids), _ptr(hs)))

    def batch_upload_part(self, total_reads, total_samples, first_read, signals, offsets, target_ids):
        """strq_batch_upload_part: reads [first_read, first_read + len(target_ids)) of a resident batch of `total_reads` int16 reads
        (`total_samples` samples in all); parts follow each other, the first one (first_read = 0) sizes the device buffers."""
        signals = np.ascontiguousarray(signals)
        if signals.dtype != np.int16:
            raise ValueError("signals must be int16")
        offsets = _c(offsets, np.int64); target_ids = _c(target_ids, np.int32)
        self._n_batch = int(total_reads)
        self._check(self._lib.strq_batch_upload_part(self._h, ctypes.c_int64(total_reads), ctypes.c_int64(total_samples), ctypes.c_int64(first_read),
                                                     ctypes.c_int64(len(target_ids)), _ptr(signals), ctypes.c_int32(0), _ptr(offsets), _ptr(target_ids)))

    def batch_run(self):
        self._check(self._lib.strq_batch_run(self._h))

    def batch_run_range(self, first, last):
        """Reads [first, last) of the uploaded batch only (strq_batch_run_range)."""
        self._check(self._lib.strq_batch_run_range(self._h, ctypes.c_int64(first), ctypes.c_int64(last)))

    def batch_fetch(self):
        out = np.zeros(self._n_batch, dtype=RESULT_DTYPE)
        self._check(self._lib.strq_batch_fetch(self._h, _ptr(out)))
        return out

    def batch_fetch_flank_ranges(self):
        """strq_batch_fetch_flank_ranges: (n, 4) int64 -- per read of the last batch the raw samples [begin, end) of the whole prefix
        flank and of the whole suffix flank: the ends of the flank alignments before the trim."""
        out = np.zeros((self._n_batch, 4), np.int64)
        self._check(self._lib.strq_batch_fetch_flank_ranges(self._h, _ptr(out), ctypes.c_int64(self._n_batch)))
        return out

    def batch_fetch_range(self, first, last):
        """Rows of reads [first, last) (strq_batch_fetch_range): waits only for the sub-batches in flight that hold them."""
        out = np.zeros(max(0, int(last) - int(first)), dtype=RESULT_DTYPE)
        self._check(self._lib.strq_batch_fetch_range(self._h, ctypes.c_int64(first), ctypes.c_int64(last), _ptr(out)))
        return out

    def detect_batch(self, signals, offsets, target_ids, host_stats=None):
        """strq_detect_batch: signals stay in this (host) buffer and are uploaded one sub-batch ahead of
        the kernels.  Use batch_upload / batch_run / batch_fetch to keep a batch resident in HBM."""
        signals = np.ascontiguousarray(signals)
        if signals.dtype == np.int16:
            dtype = 0
        elif signals.dtype == np.float64:
            dtype = 1
        else:
            raise ValueError("signals must be int16 or float64")
        offsets = _c(offsets, np.int64); target_ids = _c(target_ids, np.int32)
        hs = None if host_stats is None else _c(host_stats, np.float64)
        self._n_batch = len(target_ids)
        out = np.zeros(self._n_batch, dtype=RESULT_DTYPE)
        self._check(self._lib.strq_detect_batch(self._h, ctypes.c_int64(len(target_ids)), _ptr(signals), ctypes.c_int32(dtype),
                                                _ptr(offsets), _ptr(target_ids), _ptr(hs), _ptr(out)))
        return out

    def detect_batch_reads(self, reads, target_ids):
        """strq_detect_batch_reads: `reads` is a list of 1-D arrays, all int16 or all float64 (C-contiguous); nothing
        is concatenated on the host."""
        n = len(reads)
        if n == 0:
            return np.zeros(0, dtype=RESULT_DTYPE)
        dt = reads[0].dtype
        if dt == np.int16:
            dtype = 0
        elif dt == np.float64:
            dtype = 1
        else:
            raise ValueError("signals must be int16 or float64")
        reads = [np.ascontiguousarray(r, dtype=dt) for r in reads]          # views where possible; kept alive through the call
        ptrs = (ctypes.c_void_p * n)(*[r.ctypes.data for r in reads])
        lengths = np.array([len(r) for r in reads], np.int64)
        target_ids = _c(target_ids, np.int32)
        self._n_batch = n
        out = np.zeros(n, dtype=RESULT_DTYPE)
        self._check(self._lib.strq_detect_batch_reads(self._h, ctypes.c_int64(n), ptrs, _ptr(lengths), ctypes.c_int32(dtype),
                                                      _ptr(target_ids), None, _ptr(out)))
        return out

    # ---- scan -----------------------------------------------------------------------------
    def scan_batch_reads(self, reads, cand_ids, min_score, scores=False):
        """strq_scan_batch_reads: every read (a list of 1-D arrays, all int16 or all float64) against every candidate (target ids);
        returns (rows, winners) -- winners[i] the position of read i's winner in `cand_ids`, -1 = none -- or, with scores=True,
        (rows, winners, scores[n_reads, n_cand, 2])."""
        n = len(reads)
        cand = _c(cand_ids, np.int32)
        sc = np.zeros((n, len(cand), 2), np.float64)
        if n == 0:
            if len(cand) == 0 or not min_score > 0:
                raise StriqueHipError(STRQ_ERR_ARG, "scan: at least one candidate, min_score above 0")
            out = np.zeros(0, dtype=RESULT_DTYPE); win = np.zeros(0, np.int32)
            return (out, win, sc) if scores else (out, win)
        dt = reads[0].dtype
        if dt == np.int16:
            dtype = 0
        elif dt == np.float64:
            dtype = 1
        else:
            raise ValueError("signals must be int16 or float64")
        reads = [np.ascontiguousarray(r, dtype=dt) for r in reads]
        ptrs = (ctypes.c_void_p * n)(*[r.ctypes.data for r in reads])
        lengths = np.array([len(r) for r in reads], np.int64)
        self._n_batch = n
        out = np.zeros(n, dtype=RESULT_DTYPE); win = np.full(n, -1, np.int32)
        self._check(self._lib.strq_scan_batch_reads(self._h, ctypes.c_int64(n), ptrs, _ptr(lengths), ctypes.c_int32(dtype),
                                                    ctypes.c_int32(len(cand)), _ptr(cand), ctypes.c_double(min_score),
                                                    _ptr(out), _ptr(win), _ptr(sc) if scores else None))
        return (out, win, sc) if scores else (out, win)

    def scan_set(self, cand_ids, min_score):
        """strq_scan_set: batch_run / batch_run_range scan the uploaded reads for these candidates from now on."""
        cand = _c(cand_ids, np.int32)
        self._check(self._lib.strq_scan_set(self._h, ctypes.c_int32(len(cand)), _ptr(cand), ctypes.c_double(min_score)))
        self._n_cand = len(cand)

    def scan_clear(self):
        self._check(self._lib.strq_scan_clear(self._h))

    def batch_fetch_scan(self, scores=False):
        """Winners (and scores[n_reads, n_cand, 2]) of the last run call (strq_batch_fetch_scan)."""
        n = getattr(self, '_n_batch', 0)
        win = np.full(max(1, n), -1, np.int32); sc = np.zeros((n, getattr(self, '_n_cand', 0), 2), np.float64)
        self._check(self._lib.strq_batch_fetch_scan(self._h, _ptr(win), _ptr(sc) if scores else None))
        return (win[:n], sc) if scores else win[:n]

    def debug_conditioning(self, read, n):
        levels = np.zeros(n, np.uint8); lval = np.zeros(256, np.float32); sc = np.zeros(10)
        self._check(self._lib.strq_debug_conditioning(self._h, ctypes.c_int64(read), _ptr(levels), ctypes.c_int64(n), _ptr(lval), _ptr(sc)))
        return levels, lval, sc

    def debug_score_tables(self, level_val, classes):
        """strq_debug_score_tables: the score tables of len(classes) jobs -- level_val[j] the 256 level values, classes[j] the class
        values of job j -- built by the code strq_align_batch builds them with.  One dict per job, everything raw: 'total', 'need',
        'packed', 'n_hard' as the kernel reported them, 'entries' (of the finished table), 'band_lo' (int32 per class), 'table'
        (float32[entries]), 'hi16' / 'lo8' (the two planes of the 24-bit copy, `total` elements each) and 'handed' (the
        (class, level) pairs the kernel listed for the host)."""
        level_val = _c(level_val, np.float32).reshape(-1, 256)
        nj = len(classes)
        if nj != len(level_val):
            raise ValueError("one row of 256 level values per job")
        cls_off = np.zeros(nj + 1, np.int64)
        for j, cl in enumerate(classes):
            cls_off[j + 1] = cls_off[j] + len(cl)
        cls = np.concatenate([_c(cl, np.float32) for cl in classes])
        tot = int(cls_off[-1])
        info = np.zeros((nj, 5), np.int32); band_lo = np.zeros(tot, np.int32); table = np.zeros(256 * tot, np.float32)
        planes = np.zeros(768 * tot + 8 * nj, np.uint8)
        cap = 1 << 16
        handed = np.zeros((cap, 4), np.int32); n_handed = ctypes.c_int32(0)
        self._check(self._lib.strq_debug_score_tables(self._h, ctypes.c_int32(nj), _ptr(level_val), _ptr(cls), _ptr(cls_off), _ptr(info),
                                                      _ptr(band_lo), _ptr(table), _ptr(planes), _ptr(handed), ctypes.c_int32(cap),
                                                      ctypes.byref(n_handed)))
        handed = handed[:min(cap, n_handed.value)]
        out = []
        for j in range(nj):
            c0, k = int(cls_off[j]), int(cls_off[j + 1] - cls_off[j])
            total, need, packed, n_hard, entries = (int(v) for v in info[j])
            slot = planes[768 * c0 + 8 * j:768 * (c0 + k) + 8 * j + 8]
            lo_at = (2 * total + 3) & ~3
            out.append({"total": total, "need": need, "packed": packed, "n_hard": n_hard, "entries": entries,
                        "band_lo": band_lo[c0:c0 + k].copy(), "table": table[256 * c0:256 * c0 + entries].copy(),
                        "hi16": slot[:2 * total].view(np.uint16).copy(), "lo8": slot[lo_at:lo_at + total].copy(),
                        "handed": [(int(h[1]), int(h[2])) for h in handed if h[0] == j]})
        return out

    def _debug_scores(self, entry, nv, model_ids, xs, ws, extra):
        if not (len(model_ids) == len(xs) == len(ws)):
            raise ValueError("one model id, one stretch and one array of bounds per read")
        x, x_off = _offsets(xs, np.float64); w, w_off = _offsets(ws, np.int32)
        ids = _c(model_ids, np.int32); out = np.zeros((max(1, int(w_off[-1])), nv), np.float64); launched = np.full(2, -1, np.int32)
        self._check(getattr(self._lib, entry)(self._h, ctypes.c_int32(len(xs)), _ptr(ids), *(extra + [_ptr(x), _ptr(x_off), _ptr(w), _ptr(w_off),
                                                                                                  _ptr(out), _ptr(launched)])))
        out = out[:int(w_off[-1])]
        return [out[int(w_off[r]):int(w_off[r + 1])] for r in range(len(xs))], (int(launched[0]), int(launched[1]))

    def debug_variant_scores(self, model_ids, n_alt, xs, ws):
        """strq_debug_variant_scores: per read a model id, its stretch (float64) and its bounds (int32); one launch of the variant
        score kernel.  Returns ([(passages, n_alt + 1) float64 per read], (mode, NB) of the instance that ran)."""
        return self._debug_scores("strq_debug_variant_scores", n_alt + 1, model_ids, xs, ws, [ctypes.c_int32(n_alt)])

    def debug_mod_llr_scores(self, model_ids, xs, ws):
        """strq_debug_mod_llr_scores: the same through the kernel of the per-unit scores; (V_base, V_mod) per unit, (mode, 2)."""
        return self._debug_scores("strq_debug_mod_llr_scores", 2, model_ids, xs, ws, [])

    def debug_variant_bounds(self, model_id, n_alt, lengths, paths=None, recs=None, last=None, status=None, cap=None, guard=4):
        """strq_debug_variant_bounds: count pass and write pass of the bounds kernels for reads of `lengths` observations -- `paths`
        (one int32 state path per read: the scan route) or `recs` (T + 1 uint64 hub records per read) with `last` (the hop route);
        `status` the decode status per read (default 0), `cap` the cap of the write pass per read (default -1: the count).
        One dict per read: 'n', 'bad_count', 'bad_write', 'cap' (of the write pass), 'w', 'branch' (the `cap` entries), 'untouched'."""
        nr = len(lengths)
        off = np.zeros(nr + 1, np.int64); off[1:] = np.cumsum(lengths)
        status = _c(np.zeros(nr) if status is None else status, np.int32); cap = _c(np.full(nr, -1) if cap is None else cap, np.int32)
        stride = int(max([t // 3 + 1 for t in lengths] + [int(v) for v in cap])) + guard
        p = r = l = None
        if paths is not None:
            p, _ = _offsets(paths, np.int32)
        else:
            r, _ = _offsets(recs, np.uint64); l = _c(last, np.uint32)
        n = np.zeros(nr, np.int32); bad = np.zeros((nr, 2), np.int32); w = np.zeros((nr, stride), np.int32); br = np.zeros((nr, stride), np.int32)
        same = np.zeros(nr, np.int32)
        self._check(self._lib.strq_debug_variant_bounds(self._h, ctypes.c_int32(model_id), ctypes.c_int32(n_alt), ctypes.c_int32(nr), _ptr(off), _ptr(p),
                                                        _ptr(r), _ptr(l), _ptr(status), _ptr(cap), ctypes.c_int32(stride), ctypes.c_int32(guard),
                                                        _ptr(n), _ptr(bad), _ptr(w), _ptr(br), _ptr(same)))
        out = []
        for i in range(nr):
            k = int(cap[i]) if cap[i] >= 0 else int(n[i])
            out.append({"n": int(n[i]), "bad_count": int(bad[i, 0]), "bad_write": int(bad[i, 1]), "cap": k, "w": w[i, :k].copy(),
                        "branch": br[i, :k].copy(), "untouched": bool(same[i])})
        return out

    def debug_flank_mod_bounds(self, paths, column_of, groups, status=None):
        """strq_debug_flank_mod_bounds: one launch of the bounds kernel of the flank methylation calls.  paths: one int32 state path
        per flank stretch, all of one flank profile model; column_of: the profile column per emitting state of that model (-1 for
        none); groups: per stretch a list of (c0, c1) column ranges; status: the decode status per stretch (default: a path).
        Per stretch an (n_groups, 3) int32 array of (status, u, w) as strique_amd.flank_mod.bounds gives them."""
        nf = len(paths)
        if nf != len(groups):
            raise ValueError("one list of groups per stretch")
        p, off = _offsets(paths, np.int32)
        col = _c(column_of, np.int32)
        g_off = np.zeros(nf + 1, np.int64); g_off[1:] = np.cumsum([len(g) for g in groups])
        flat = _c([c for g in groups for c in g] or [(0, 0)], np.int32).reshape(-1, 2)
        st = None if status is None else _c(status, np.int32)
        if st is not None and len(st) != nf:
            raise ValueError("one decode status per stretch")
        out = np.zeros((max(1, int(g_off[-1])), 3), np.int32)
        self._check(self._lib.strq_debug_flank_mod_bounds(self._h, ctypes.c_int32(nf), _ptr(off), _ptr(p), _ptr(st), ctypes.c_int32(len(col)), _ptr(col),
                                                          _ptr(g_off), _ptr(flat), _ptr(out)))
        return [out[int(g_off[f]):int(g_off[f + 1])].copy() for f in range(nf)]

    def debug_filtered(self, read, n, dtype=np.int16):
        """strq_debug_filtered: the first `n` median-filtered samples of read `read` of the last sub-batch; `dtype` is the
        element type of the batch (int16 or float64)."""
        out = np.zeros(n, np.dtype(dtype))
        if out.dtype not in (np.dtype(np.int16), np.dtype(np.float64)):
            raise ValueError("dtype must be int16 or float64")
        self._check(self._lib.strq_debug_filtered(self._h, ctypes.c_int64(read), _ptr(out), ctypes.c_int64(n)))
        return out


RESULT_DTYPE = np.dtype([("count", np.int32), ("status", np.int32), ("score_prefix", np.float64),
                         ("score_suffix", np.float64), ("log_p", np.float64), ("offset", np.int64),
                         ("ticks", np.int64), ("prefix_begin", np.int64), ("prefix_end", np.int64),
                         ("suffix_begin", np.int64), ("suffix_end", np.int64)], align=True)

RENORM_FIT_DTYPE = np.dtype([("a", np.int32), ("b", np.int32), ("w", np.int32), ("fitted", np.int32), ("score", np.int64)], align=True)
RENORM_DTYPE = np.dtype([("applied", np.int32), ("pad_", np.int32), ("fit", RENORM_FIT_DTYPE, (3,))], align=True)

FLANK_MOD_DTYPE = np.dtype([("flank", np.int32), ("pos", np.int32), ("n_sites", np.int32), ("n_columns", np.int32), ("status", np.int32), ("pad_", np.int32),
                            ("begin", np.int64), ("end", np.int64), ("v_base", np.float64), ("v_mod", np.float64)], align=True)
TRACTS_DTYPE = np.dtype([("status", np.int32), ("n_tracts", np.int32), ("count", np.int32, (3,)), ("pad_", np.int32), ("log_p", np.float64)], align=True)
MOTIFS_DTYPE = np.dtype([("status", np.int32), ("n_cand", np.int32), ("n_seg", np.int64), ("majority", np.int32), ("decode_status", np.int32),
                         ("begin", np.int64), ("end", np.int64), ("obs_won", np.int64, (4,)), ("count_m", np.int32), ("pad_", np.int32),
                         ("log_p_m", np.float64)], align=True)
ANCHORED_DTYPE = np.dtype([("kind", np.int32), ("status", np.int32), ("count", np.int32), ("pad_", np.int32), ("log_p", np.float64),
                           ("begin", np.int64), ("end", np.int64), ("free_samples", np.int64)], align=True)
