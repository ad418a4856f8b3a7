"""Lines of character quads for the spine tests (tests/test_cpu_spines.py, tests/test_gpu_spines.py): corners as ``(y, x)``
rows in the order up-left, up-right, down-right, down-left (tests/strip_cases.py)."""
import numpy as np

from tests import strip_cases as C


def straight(count=12, width=16.0, height=20.0, at=(60.0, 40.0), angle=0.0, mirrored=False):
    """``count`` equal characters side by side, the first one's left edge centred at ``at``, read along ``angle``."""
    A = np.array([np.sin(angle), np.cos(angle)])
    quads = np.stack([C.rect(*(np.asarray(at) + A * width * (k + 0.5)), width, height, angle) for k in range(count)])
    return quads[:, [1, 0, 3, 2]][::-1] if mirrored else quads


def arc(centre=(20.0, 20.0), R=200.0, count=20, width=12.0, height=20.0, s=15.7, first=0.04, scale=1.0):
    """``count`` characters whose centres lie ``s`` pixels apart on the circle of radius ``R`` about ``centre``, each along
    the circle's tangent with its top towards the centre: the line starts below the centre, reads to the right and bends
    upwards.  Everything times ``scale``."""
    quads = []
    for k in range(count):
        t = first + k * s / R                                   # the angle from straight below the centre
        c = np.asarray(centre) + R * np.array([np.cos(t), np.sin(t)])
        quads.append(C.rect(c[0], c[1], width, height, -t))
    return np.stack(quads) * scale


def radial_image(shape, centre, R, gain=4.0):
    """clip(rint(128 + gain * (r - R))) with r the distance of the pixel's centre from ``centre``, on all three channels."""
    y, x = np.mgrid[:shape[0], :shape[1]] + 0.5
    r = np.hypot(y - centre[0], x - centre[1])
    v = np.clip(np.rint(128 + gain * (r - R)), 0, 255).astype(np.uint8)
    return np.repeat(v[:, :, None], 3, axis=2)
