"""Records for the tests of the granule kernel's routing (tests/test_gpu_gran_route.py and its CPU twin in
tests/test_gran_route_emul.py): the generator's frames with ONE edit planted at a chosen frame -- every fact a wave of
k_decode_g routes by (pdmp3_amd/csrc/decode_core.h GranRoute) changed where a workgroup begins, ends, and in between."""
import numpy as np

from corpus import FR_MODE_SHIFT, FR_MODEEXT_SHIFT, FR_RESET, GC_WIN_SWITCH, GC_BLOCK_TYPE_SHIFT, MODE_JOINT, MODE_MONO

FR_MODE_MASK = 3 << FR_MODE_SHIFT

# edit -> needs a frame before the planted one
EDITS = {"mono": False, "stereo_after_mono": True, "reset": True, "intensity": False, "lsf": False, "h5": False,
         "frame0_reset": False, "frame0_no_reset": False}


def _set_mode(sd, f, mode, ext0=None):
    fr = sd["frame"][f]
    fr[...] = (fr & ~np.uint8(FR_MODE_MASK)) | np.uint8(mode << FR_MODE_SHIFT)
    if ext0 is not None:
        fr[...] = (fr & ~np.uint8(1 << FR_MODEEXT_SHIFT)) | np.uint8(ext0 << FR_MODEEXT_SHIFT)


def plant(sd, edit, f):
    """-> a copy of the records sd [n][2][2] with `edit` at frame f (frame0_*: at frame 0 whatever f), or None where the
    edit needs a frame the launch does not have"""
    sd = sd.copy()
    if EDITS[edit] and f == 0:
        return None
    if edit == "mono":
        _set_mode(sd, f, MODE_MONO)
    elif edit == "stereo_after_mono":
        _set_mode(sd, f - 1, MODE_MONO)
        assert ((sd["frame"][f, 0, 0] >> FR_MODE_SHIFT) & 3) != MODE_MONO
    elif edit == "reset":
        sd["frame"][f] |= np.uint8(FR_RESET)
    elif edit == "intensity":
        _set_mode(sd, f, MODE_JOINT, 1)
    elif edit == "lsf":
        sd["lsf"][f] = 1
    elif edit == "h5":
        sd["flags"][f, 1, 1] = (sd["flags"][f, 1, 1] & ~np.uint8(GC_WIN_SWITCH | (3 << GC_BLOCK_TYPE_SHIFT))) | np.uint8(GC_WIN_SWITCH | (2 << GC_BLOCK_TYPE_SHIFT))
    elif edit == "frame0_reset":
        sd["frame"][0] |= np.uint8(FR_RESET)
    elif edit == "frame0_no_reset":
        sd["frame"][0] &= ~np.uint8(FR_RESET)
    else:
        raise KeyError(edit)
    return sd


def positions(n, wpw):
    """frames of a launch of n frames at which an edit is planted: the first, an inner and the last frame of a workgroup of
    wpw waves (wpw / 2 frames) -- the launch's first workgroup, one in its middle and its last one (the last may be partial)"""
    fpw = wpw // 2
    groups = sorted({0, ((n - 1) // fpw) // 2, (n - 1) // fpw})
    out = []
    for k in groups:
        a, b = k * fpw, min(n, (k + 1) * fpw) - 1
        for f in sorted({a, (a + b) // 2, b}):
            if f not in out:
                out.append(f)
    return out


def streams(sd, wpw):
    """every (edit, frame, records) of a launch: the unedited records first"""
    n = sd.shape[0]
    yield "plain", -1, sd
    for edit in EDITS:
        for f in ([0] if edit.startswith("frame0") else positions(n, wpw)):
            e = plant(sd, edit, f)
            if e is not None:
                yield edit, f, e
