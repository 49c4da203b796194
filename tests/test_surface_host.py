"""The eigen-solver of lv_surface.hpp (sym3_eig, what lv_map_normals runs per point) compiled for the host and held to
numpy.linalg.eigh on seeded covariance matrices: rank 0, 1, 2, isotropic and generic ones at scales from 1e-12 to 1e+6.

Bounds: eigenvalues within 8 eps64 trace; the l0 eigenvector within 8 eps64 l2 / (l1 - l0) rad wherever (l1 - l0) / l2 >= 1e-3
(the first-order perturbation bound of a simple eigenvector; the constants are rounding-count margins: the issue's 64 for the vector
tightened to 8, the same count as for the values, which the solver allows)."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "limo-velo_amd", "csrc")
EPS = np.finfo(np.float64).eps

DRIVER = r'''
#define LV_SURFACE_HOST_ONLY 1
#include "lv_surface.hpp"
#include <stdio.h>
int main() {
    double c[6], l[3], v[3];
    while (fread(c, sizeof(double), 6, stdin) == 6) {
        lv::sym3_eig(c, l, v);
        fwrite(l, sizeof(double), 3, stdout);
        fwrite(v, sizeof(double), 3, stdout);
        float n[3], cv;
        lv::surf_normal(c[0], c[1], c[2], c[3], c[4], c[5], 5, 5, 0, 0.0, 0.0, 0.0, n[0], n[1], n[2], cv);
        double o[4] = {n[0], n[1], n[2], cv};
        fwrite(o, sizeof(double), 4, stdout);
    }
    return 0;
}
'''


@pytest.fixture(scope="module")
def solver(tmp_path_factory):
    d = tmp_path_factory.mktemp("surface_host")
    src = d / "driver.cpp"
    src.write_text(DRIVER)
    exe = d / "driver"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", CSRC, str(src), "-o", str(exe)])

    def run(C):
        C = np.asarray(C, np.float64)
        packed = np.stack([C[:, 0, 0], C[:, 0, 1], C[:, 0, 2], C[:, 1, 1], C[:, 1, 2], C[:, 2, 2]], axis=1)
        out = subprocess.run([str(exe)], input=np.ascontiguousarray(packed).tobytes(), stdout=subprocess.PIPE, check=True).stdout
        r = np.frombuffer(out, np.float64).reshape(-1, 10)
        return r[:, :3], r[:, 3:6], r[:, 6:9], r[:, 9]

    return run


def _rot(rng, n):
    q, _ = np.linalg.qr(rng.standard_normal((n, 3, 3)))
    return q


def _cases():
    rng = np.random.default_rng(20240607)
    out = []
    for scale in (1e-12, 1e-9, 1e-6, 1e-3, 1.0, 1e3, 1e6):
        n = 400
        Q = _rot(rng, n)
        ev = np.sort(rng.uniform(0, 1, (n, 3)), axis=1)
        ev[:50, 0] = 0.0                           # rank 2
        ev[50:100, :2] = 0.0                       # rank 1
        ev[100:120] = 0.0                          # rank 0
        ev[120:150] = ev[120:150, 2:3]             # isotropic
        ev[150:200, 0] *= 1e-6                     # a flat patch: the common case on a surface
        ev[200:230, 1] = ev[200:230, 2]            # l1 = l2: the normal is still simple
        C = np.einsum("nij,nj,nkj->nik", Q, ev * scale, Q)
        out.append(0.5 * (C + np.transpose(C, (0, 2, 1))))
        # covariances of actual neighbourhoods: 10 points on a noisy plane
        pts = rng.standard_normal((n, 10, 3)) * np.array([1.0, 1.0, 0.01]) * np.sqrt(scale)
        pts = np.einsum("nij,nkj->nki", Q, pts)
        d = pts - pts.mean(axis=1, keepdims=True)
        out.append(np.einsum("nki,nkj->nij", d, d) / 10)
    axes = np.zeros((3, 3, 3))
    for a in range(3):
        axes[a, a, a] = 2.5                        # exactly diagonal, rank 1
    out.append(axes)
    out.append(np.diag([3.0, 1.0, 2.0])[None])
    return np.concatenate(out)


def test_eigenvalues_and_normal_against_eigh(solver):
    C = _cases()
    l, v, nrm, curv = solver(C)
    lam, vec = np.linalg.eigh(C)
    tr = np.abs(lam).sum(axis=1)
    err = np.abs(l - lam).max(axis=1)
    print("eigenvalue error / (eps trace): max", np.max(err[tr > 0] / (EPS * tr[tr > 0])))
    assert np.all(err <= 8 * EPS * tr), np.max(err[tr > 0] / (EPS * tr[tr > 0]))
    assert np.all(l[:, 0] <= l[:, 1]) and np.all(l[:, 1] <= l[:, 2])
    assert np.allclose(np.linalg.norm(v, axis=1), 1.0, rtol=0, atol=8 * EPS)
    with np.errstate(divide="ignore", invalid="ignore"):
        gap = np.where(lam[:, 2] > 0, (lam[:, 1] - lam[:, 0]) / lam[:, 2], 0.0)
    sel = gap >= 1e-3
    assert sel.sum() > 0.5 * len(C)
    ang = np.arcsin(np.minimum(np.linalg.norm(np.cross(v[sel], vec[sel][:, :, 0]), axis=1), 1.0))
    bound = 8 * EPS / gap[sel]
    print("eigenvector error / bound: max", np.max(ang / bound), "points", int(sel.sum()))
    assert np.all(ang <= bound), np.max(ang / bound)
    # the normal: v signed so that its largest component is positive, rounded to f32; the curvature l0 / trace
    big = np.abs(nrm[sel]).argmax(axis=1)
    assert np.all(nrm[sel][np.arange(sel.sum()), big] > 0)
    assert np.all(np.abs(np.abs(nrm[sel]) - np.abs(v[sel])) <= 2.0 ** -24)
    pos = tr > 0
    assert np.all(np.abs(curv[pos] - lam[pos, 0] / lam[pos].sum(axis=1)) <= 1e-7 + 16 * EPS)
    assert np.all(curv[~pos] == 0)


def test_too_few_neighbours_give_a_zero_normal(solver, tmp_path):
    src = tmp_path / "few.cpp"
    src.write_text('#define LV_SURFACE_HOST_ONLY 1\n#include "lv_surface.hpp"\n#include <stdio.h>\nint main(){double c[6]={1,0,0,1,0,1};float n[3],cv;'
                   'lv::surf_normal(c[0],c[1],c[2],c[3],c[4],c[5],2,3,0,0,0,0,n[0],n[1],n[2],cv);printf("%g %g %g %d\\n",n[0],n[1],n[2],cv!=cv);'
                   'double d[6]={1,0,0,1,0,1e-3};lv::surf_normal(d[0],d[1],d[2],d[3],d[4],d[5],9,3,1,0,0,-5,n[0],n[1],n[2],cv);printf("%g\\n",n[2]);return 0;}')
    exe = tmp_path / "few"
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", CSRC, str(src), "-o", str(exe)])
    a, b = subprocess.check_output([str(exe)]).decode().split("\n")[:2]
    assert a.split() == ["0", "0", "0", "1"]
    assert float(b) == -1.0   # orient 1: towards the viewpoint below
