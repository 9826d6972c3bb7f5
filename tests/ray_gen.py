"""Ray generators shared by the GPU parity tests and the host-walk tests."""
import numpy as np


def random_rays(n, seed, span=15.0):
    rng = np.random.default_rng(seed)
    o = rng.uniform(-span, span, (n, 3)).astype(np.float32)
    o[:, 1] = np.abs(o[:, 1]) + 0.5
    d = rng.normal(size=(n, 3)).astype(np.float32)
    return np.concatenate([o, d], 1)


def camera_rays(cam, n, seed):
    """Primary rays in the camera frustum (Camera::ray with jitter, world.rs:53-63)."""
    rng = np.random.default_rng(seed)
    f = cam.fields()
    org, llc, hor, ver = f[0:3], f[3:6], f[6:9], f[9:12]
    s = rng.random(n, dtype=np.float32)[:, None]
    t = rng.random(n, dtype=np.float32)[:, None]
    d = (((llc + hor * s) + ver * t) - org).astype(np.float32)
    return np.concatenate([np.broadcast_to(org, (n, 3)), d], 1).astype(np.float32)
