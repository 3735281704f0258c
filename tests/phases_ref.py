"""What the frame-phase tests share: the phase counts and the clip lengths of the batch cases."""

PHASES_ALL = (1, 2, 4, 8, 16, 32)


def lengths_of(window, stride, phases):
    """name -> samples.  The issue's lengths -- window + 255 strides and its neighbours -- and the same one stride later, where the
    reference's count (LBAudioDetective.m:250-255: (L - window) / stride / 128, one window short of the windows that fit) makes
    count_0 two and every other phase's count one."""
    h = 128 // phases
    out = {}
    for tag, base in (("w255", window + 255 * stride), ("w256", window + 256 * stride)):
        out[tag] = base
        out[tag + "_last_gains"] = base + (128 - h) * stride
        out[tag + "_last_gains_m1"] = base + (128 - h) * stride - 1
    out["one_frame"] = window + 128 * stride          # count_0 = 1, nothing at any other phase
    out["one_frame_m1"] = window + 128 * stride - 1   # nothing at all
    out["short"] = window - 1                         # shorter than a window
    return out


