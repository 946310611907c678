"""Device augmentation throughput at the benchmark patch: loader-sized batch (B=2, basic_generator_patch_size) -> 48x192x192.
--elastic adds the elastic-deformation leg (every sample deformed, sigma 13 = radius 52, the widest filter of the reference's range):
the whole call and its stages apart (noise, the three blur passes, the warp) by device events; --host adds the reference's
computation of the same shape with scipy in float64 (3 x gaussian_filter + map_coordinates per sample); --json FILE keeps the
measured lines."""
import argparse, json, sys, os, time
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
import numpy as np
import torch
from multitalent_amd.training.data_augmentation.spatial import SpatialTransformDevice, MirrorTransformDevice, get_patch_size
from multitalent_amd.training.data_augmentation.color import default_3d_augmentation_params, GammaDevice
ap = argparse.ArgumentParser()
ap.add_argument('--elastic', action='store_true')
ap.add_argument('--host', action='store_true')
ap.add_argument('--intensity', action='store_true')
ap.add_argument('--json', default=None)
args = ap.parse_args()
dev = torch.device('cuda:0')
p = default_3d_augmentation_params()
ps = (48, 192, 192)
bps = tuple(int(i) for i in get_patch_size(ps, p['rotation_x'], p['rotation_y'], p['rotation_z'], (0.85, 1.25)))
x = torch.randn((2, 1) + bps, device=dev); s = torch.randint(0, 5, (2, 1) + bps, device=dev).float()
st = SpatialTransformDevice(ps, angle_x=p['rotation_x'], angle_y=p['rotation_y'], angle_z=p['rotation_z'], scale=p['scale_range'],
                            p_rot_per_sample=1.0, p_scale_per_sample=1.0, border_cval_seg=-1)     # every sample resampled: worst case
np.random.seed(0)
st(x, s); torch.cuda.synchronize()
t = time.time(); n = 10
for _ in range(n):
    d, g = st(x, s)
torch.cuda.synchronize()
dt = (time.time() - t) / n
print('loader patch %s -> %s, B=2, order 3 data + per-label order 1 seg, every sample rotated+scaled: %.2f ms per batch (%.0f patches/s)' % (bps, ps, dt * 1e3, 2 / dt))
gm = GammaDevice(p_per_sample=1.0); mr = MirrorTransformDevice()
t = time.time()
for _ in range(n):
    d2 = gm(d.clone()); mr(d2, g.clone())
torch.cuda.synchronize()
print('gamma (retain stats) + mirror on every sample: %.2f ms per batch' % ((time.time() - t) / n * 1e3))
lines = [{'leg': 'spatial', 'loader_patch': list(bps), 'patch': list(ps), 'batch': 2, 'ms_per_batch': dt * 1e3}]


def timed(fn, n=10, warm=2):
    """median and spread of n device-event timings of fn() after `warm` untimed calls, in ms."""
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


if args.elastic:
    from multitalent_amd import _lib
    from multitalent_amd.training.data_augmentation.spatial import elastic_noise, warp_sample
    HBM_PEAK = 8.0e12                     # bytes/s, the MI355X's specified HBM3E peak
    el = SpatialTransformDevice(ps, angle_x=p['rotation_x'], angle_y=p['rotation_y'], angle_z=p['rotation_z'], scale=p['scale_range'],
                                p_rot_per_sample=1.0, p_scale_per_sample=1.0, border_cval_seg=-1, do_elastic_deform=True,
                                p_el_per_sample=1.0, alpha=p['elastic_deform_alpha'], sigma=(13., 13.))
    np.random.seed(0)
    med, lo, hi = timed(lambda: el(x, s))
    print('elastic, every sample deformed (sigma 13, radius 52) + rotated + scaled: %.2f ms per batch (min %.2f, max %.2f; %.0f patches/s)'
          % (med, lo, hi, 2e3 / med))
    lines.append({'leg': 'elastic_whole_call', 'ms_per_batch': med, 'min_ms': lo, 'max_ms': hi})
    seeds = [e[2] for e in el.last_elastic]
    med, lo, hi = timed(lambda: torch.cat([elastic_noise(sd, 3, ps, dev) for sd in seeds]))
    print('  noise (2 x 3 x patch, seeded device generator): %.3f ms (min %.3f, max %.3f)' % (med, lo, hi))
    lines.append({'leg': 'elastic_noise', 'ms': med, 'min_ms': lo, 'max_ms': hi})
    noise = torch.cat([elastic_noise(sd, 3, ps, dev) for sd in seeds])
    tmp = torch.empty_like(noise)
    sg = np.full(6, 13., dtype=np.float32)
    lib, stream = _lib.load(), torch.cuda.current_stream().cuda_stream
    nbytes = 2 * 4 * noise.numel()          # one read and one write per element
    for axis, name in enumerate('DHW'):
        med, lo, hi = timed(lambda: _lib.check(lib.mt_gaussian_blur_axis_zero(noise.data_ptr(), tmp.data_ptr(), 6, ps[0], ps[1], ps[2], axis,
                                                                              sg.ctypes.data_as(_lib.c_float_p), stream), 'blur'))
        print('  blur pass along %s (6 channels of %s, 105 taps): %.3f ms (min %.3f, max %.3f) = %.2f TB/s of one read + one write, %.0f %% of the %.1f TB/s HBM peak'
              % (name, ps, med, lo, hi, nbytes / med * 1e-9, 100 * nbytes / (med * 1e-3) / HBM_PEAK, HBM_PEAK * 1e-12))
        lines.append({'leg': 'elastic_blur_' + name, 'ms': med, 'min_ms': lo, 'max_ms': hi, 'bytes': nbytes,
                      'bytes_per_s': nbytes / (med * 1e-3), 'share_of_hbm_peak': nbytes / (med * 1e-3) / HBM_PEAK})
    field, alpha = el.elastic_field(el.last_elastic, dev)
    mats = el.last_mats
    med, lo, hi = timed(lambda: (warp_sample(x, mats, ps, 3, field, alpha, 0), warp_sample(s, mats, ps, 1, field, alpha, -1, is_seg=True)))
    print('  warp (prefilter + order-3 data, per-label order-1 seg): %.2f ms (min %.2f, max %.2f)' % (med, lo, hi))
    lines.append({'leg': 'elastic_warp', 'ms': med, 'min_ms': lo, 'max_ms': hi})
    if args.host:
        from scipy import ndimage
        rs = np.random.RandomState(0)
        xh = x[0, 0].cpu().numpy().astype(np.float64)
        t0 = time.time()
        off = [ndimage.gaussian_filter(rs.random_sample(ps) * 2 - 1, 13., mode='constant', cval=0) * 450. for _ in range(3)]
        t1 = time.time()
        g = np.stack(np.meshgrid(*[np.arange(k) - (k - 1) / 2. for k in ps], indexing='ij')) + np.stack(off)
        m, ctr = mats[0, :9].reshape(3, 3).astype(np.float64), mats[0, 9:].astype(np.float64)
        co = (m @ g.reshape(3, -1) + ctr[:, None]).reshape((3,) + ps)
        t2 = time.time()
        ndimage.map_coordinates(xh, co, order=3, mode='constant', cval=0.0)
        t3 = time.time()
        print('  host, scipy float64, ONE sample: 3 x gaussian_filter %.0f ms + map_coordinates(order 3) %.0f ms = %.0f ms (a batch of 2: %.0f ms)'
              % ((t1 - t0) * 1e3, (t3 - t2) * 1e3, (t1 - t0 + t3 - t2) * 1e3, 2 * (t1 - t0 + t3 - t2) * 1e3))
        lines.append({'leg': 'elastic_host_scipy_float64_per_sample', 'gaussian_filter_x3_ms': (t1 - t0) * 1e3,
                      'map_coordinates_ms': (t3 - t2) * 1e3})
if args.intensity:
    from multitalent_amd import ops
    from multitalent_amd.training.data_augmentation import color
    from multitalent_amd.training.data_augmentation.color import _range_pick
    HBM_PEAK = 8.0e12                     # bytes/s, the MI355X's specified HBM3E peak

    # The baseline leg: the torch formulation these transforms had before the kernels (per (sample, channel) loops of elementwise
    # torch operations whose statistics are read to the host with float()), kept here only to be measured against.
    class TorchBrightness:
        def __init__(self, r=(0.75, 1.25), p=1.0):
            self.r, self.p = r, p

        def __call__(self, data):
            for b in range(data.shape[0]):
                if np.random.uniform() < self.p:
                    for c in range(data.shape[1]):
                        data[b, c] *= np.random.uniform(self.r[0], self.r[1])
            return data

    class TorchContrast:
        def __init__(self, r=(0.75, 1.25), p=1.0):
            self.r, self.p = r, p

        def __call__(self, data):
            for b in range(data.shape[0]):
                if np.random.uniform() < self.p:
                    for c in range(data.shape[1]):
                        v = data[b, c]
                        f = _range_pick(self.r[0], self.r[1])
                        mn, lo, hi = v.mean(), v.min(), v.max()
                        v.sub_(mn).mul_(f).add_(mn)
                        v.clamp_(min=float(lo), max=float(hi))
            return data

    class TorchGamma:
        def __init__(self, r=(0.7, 1.5), invert=False, p=1.0, eps=1e-7):
            self.r, self.invert, self.p, self.eps = r, invert, p, eps

        def __call__(self, data):
            for b in range(data.shape[0]):
                if np.random.uniform() < self.p:
                    if self.invert:
                        data[b].neg_()
                    for c in range(data.shape[1]):
                        v = data[b, c]
                        mn, sd = float(v.mean()), float(v.std(unbiased=False))
                        g = _range_pick(self.r[0], self.r[1])
                        lo = float(v.min())
                        rng = float(v.max()) - lo
                        v.sub_(lo).div_(rng + self.eps).pow_(g).mul_(rng).add_(lo)
                        v.sub_(float(v.mean()))
                        v.div_(float(v.std(unbiased=False)) + 1e-8).mul_(sd).add_(mn)
                    if self.invert:
                        data[b].neg_()
            return data

    def chain(ts):
        def run(d):
            for t in ts:
                d = t(d)
            return d
        return run

    def one_call(fn, xw, x0):
        """(device-event ms, host ms until fn returns) of fn(xw) on a fresh copy of x0 with an empty queue."""
        xw.copy_(x0)
        torch.cuda.synchronize()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0 = time.perf_counter()
        a.record(); fn(xw); b.record()
        host = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        return a.elapsed_time(b), host

    def stat(v):
        return {'median': float(np.median(v)), 'min': float(min(v)), 'max': float(max(v))}

    ROUNDS, CALLS, WARM = 3, 10, 3
    for Cn in (1, 4):
        x0 = torch.randn((2, Cn) + ps, device=dev) * 2 + 1
        xw = torch.empty_like(x0)
        nel = x0.numel()
        new = {'brightness': color.BrightnessMultiplicativeDevice(p_per_sample=1.), 'contrast': color.ContrastAugmentationDevice(p_per_sample=1.),
               'gamma_inverted_retain_stats': color.GammaDevice(p['gamma_range'], True, True, True, 1.),
               'gamma_retain_stats': color.GammaDevice(p['gamma_range'], False, True, True, 1.)}
        old = {'brightness': TorchBrightness(), 'contrast': TorchContrast(), 'gamma_inverted_retain_stats': TorchGamma(p['gamma_range'], True),
               'gamma_retain_stats': TorchGamma(p['gamma_range'], False)}
        new['all_four'], old['all_four'] = chain(list(new.values())), chain(list(old.values()))
        print('intensity transforms, B=2, C=%d, %s, every probability 1: %d rounds alternating kernels / torch formulation, %d calls each'
              % (Cn, ps, ROUNDS, CALLS))
        for name in new:
            res = {'kernels': ([], [], []), 'torch': ([], [], [])}        # device ms, host ms, per-round medians of the device ms
            for rnd in range(ROUNDS):
                for leg, fn in (('kernels', new[name]), ('torch', old[name])):
                    np.random.seed(rnd)
                    for _ in range(WARM if rnd == 0 else 1):
                        one_call(fn, xw, x0)
                    ts = [one_call(fn, xw, x0) for _ in range(CALLS)]
                    res[leg][0].extend(t[0] for t in ts); res[leg][1].extend(t[1] for t in ts)
                    res[leg][2].append(float(np.median([t[0] for t in ts])))
            line = {'leg': 'intensity_' + name, 'batch': 2, 'channels': Cn, 'patch': list(ps)}
            for leg in res:
                dv, ho = stat(res[leg][0]), stat(res[leg][1])
                print('  %-28s %-7s device %.3f ms (min %.3f, max %.3f; round medians %s), host until return %.3f ms (min %.3f, max %.3f)'
                      % (name, leg, dv['median'], dv['min'], dv['max'], ' '.join('%.3f' % m for m in res[leg][2]), ho['median'], ho['min'], ho['max']))
                line[leg] = {'device_ms': dv, 'device_ms_round_medians': res[leg][2], 'host_ms_until_return': ho}
            lines.append(line)
        # the two kernels on their own, BURST calls back to back between one pair of events (an upper bound of the kernel time: it
        # includes the launch gaps; rocprofv3 --kernel-trace gives the kernels alone).  Algorithmic bytes from the shape: 4 per
        # element for a statistics pass, 8 for an apply pass.  The ops are chosen so that repeating them in place keeps the values
        # in range (multiplier 1; the power maps [min, max] of the fixed statistics onto itself).
        BURST = 20
        st = ops.channel_stats(x0)
        every = np.ones(2 * Cn, dtype=bool)

        def records(op, a):
            return color._records(every, op, np.full(2 * Cn, a), 0, 1e-7)
        for kname, nbytes, fn in (('channel_stats', 4 * nel, lambda d: ops.channel_stats(d, None, st)),
                                  ('apply_scale', 8 * nel, lambda d: ops.intensity_apply(d, records(ops.INTENSITY_SCALE, 1.))),
                                  ('apply_gamma', 8 * nel, lambda d: ops.intensity_apply(d, records(ops.INTENSITY_GAMMA, 1.3), st)),
                                  ('apply_restore', 8 * nel, lambda d: ops.intensity_apply(d, records(ops.INTENSITY_RESTORE, 0.), st, st))):
            ts = []
            for i in range(WARM + CALLS):
                xw.copy_(x0)
                torch.cuda.synchronize()
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                for _ in range(BURST):
                    fn(xw)
                b.record()
                torch.cuda.synchronize()
                if i >= WARM:
                    ts.append(a.elapsed_time(b) / BURST)
            dv = stat(ts)
            print('  kernel %-14s %.4f ms per call in bursts of %d (min %.4f, max %.4f) = %.2f TB/s of %d algorithmic bytes, %.0f %% of the %.1f TB/s HBM peak'
                  % (kname, dv['median'], BURST, dv['min'], dv['max'], nbytes / dv['median'] * 1e-9, nbytes,
                     100 * nbytes / (dv['median'] * 1e-3) / HBM_PEAK, HBM_PEAK * 1e-12))
            lines.append({'leg': 'intensity_kernel_' + kname, 'batch': 2, 'channels': Cn, 'patch': list(ps), 'ms_per_call': dv, 'burst': BURST,
                          'bytes': nbytes, 'bytes_per_s': nbytes / (dv['median'] * 1e-3), 'share_of_hbm_peak': nbytes / (dv['median'] * 1e-3) / HBM_PEAK})
if args.json:
    with open(args.json, 'w') as f:
        for l in lines:
            f.write(json.dumps(l) + '\n')
