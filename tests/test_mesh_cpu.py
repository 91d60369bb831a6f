"""Host side of generate_dataset: the definition's generator against Random123's known answers, the native OFF / OBJ reader
(csrc/mesh_io.cpp) and the reference's function surface.  No GPU."""
import inspect

import numpy as np
import pytest

import mesh_reference as mr
from pcgcv2_amd import generate_dataset as gd
from pcgcv2_amd._lib import PcgcError


@pytest.mark.parametrize('ctr,key,out', mr.KNOWN_ANSWERS)
def test_philox_known_answers(ctr, key, out):
    got = mr.philox(np.array([ctr], dtype=np.uint32), key)
    assert [int(x) for x in got[0]] == list(out)


def test_uniforms_are_exact_and_in_range():
    u0, u, v = mr.uniforms(2 ** 40 + 7, 2 ** 32 - 5, 10)
    assert ((u0 >= 0) & (u0 < 1)).all() and ((u > 0) & (u < 1)).all() and ((v > 0) & (v < 1)).all()
    assert (u0 * 2.0 ** 52 == np.floor(u0 * 2.0 ** 52)).all() and (u * 2.0 ** 33 == np.floor(u * 2.0 ** 33)).all()
    a = mr.uniforms(2 ** 40 + 7, 2 ** 32 - 5, 10)[1][5:]                     # sample i depends on (seed, i) alone, across the carry
    assert np.array_equal(a, mr.uniforms(2 ** 40 + 7, 2 ** 32, 5)[1])


CUBE_FAN = [(0, 2, 3), (0, 3, 1), (4, 5, 7), (4, 7, 6), (0, 1, 5), (0, 5, 4), (2, 6, 7), (2, 7, 3), (0, 4, 6), (0, 6, 2), (1, 3, 7), (1, 7, 5)]


def test_off_cube_of_quads_is_fanned(tmp_path):
    p = tmp_path / 'cube.off'
    mr.write_off(p, mr.CUBE_VERTS, mr.CUBE_QUADS)
    verts, faces = gd.read_mesh(str(p))
    assert verts.dtype == np.float64 and faces.dtype == np.int32
    assert np.array_equal(verts, mr.CUBE_VERTS)
    assert faces.tolist() == [list(t) for t in CUBE_FAN]


def test_off_glued_header_comments_and_blank_lines(tmp_path):
    p = tmp_path / 'glued.off'
    mr.write_off(p, mr.CUBE_VERTS, mr.CUBE_QUADS, glued=True)
    assert open(p).readline() == 'OFF8 6 0\n'
    a = gd.read_mesh(str(p))
    q = tmp_path / 'commented.off'
    lines = open(p).read().split('\n')
    q.write_text('# a cube\n\n' + lines[0] + '   # counts\n\n' + '\n'.join(lines[1:5]) + '\n# half way\n\n' + '\n'.join(lines[5:])
                 + '\n\n')
    b = gd.read_mesh(str(q))
    r = tmp_path / 'one_line.off'                        # "OFF 8 6 0" on one line, a pentagon and trailing colour values
    r.write_text('OFF 5 1 0\n0 0 0 255 0 0\n1 0 0\n2 1 0\n1 2 0\n0 1 0\n5 0 1 2 3 4 0.5 0.5 0.5\n')
    v, f = gd.read_mesh(str(r))
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert np.array_equal(a[1], mr.fan(mr.CUBE_QUADS))
    assert v.shape == (5, 3) and f.tolist() == [[0, 1, 2], [0, 2, 3], [0, 3, 4]]


def test_obj_token_forms_negative_indices_and_skipped_records(tmp_path):
    p = tmp_path / 'm.obj'
    p.write_text('# comment\nmtllib x.mtl\no thing\n\nv 0 0 0\nv 1 0 0\nv 1 1 0\nv 0 1 0\nvt 0.5 0.5\nvn 0 0 1\n'
                 'g grp\nusemtl m\ns off\n'
                 'f 1 2 3\n'                              # a
                 'f 1/1 3/1 4/1\n'                        # a/b
                 'f 1/1/1 2/1/1 4/1/1\n'                  # a/b/c
                 'f 2//1 3//1 4//1\n'                     # a//c
                 'v 0.5 0.5 1.25 1.0\n'                   # (x y z w)
                 'f -1 -5 -4\n'                           # relative: 5th, 1st, 2nd
                 'f -1/-1/-1 2//1 3 4/1\n'                # mixed forms, a quad -> fan
                 '\n')
    verts, faces = gd.read_mesh(str(p))
    assert verts.tolist() == [[0, 0, 0], [1, 0, 0], [1, 1, 0], [0, 1, 0], [0.5, 0.5, 1.25]]
    assert faces.tolist() == [[0, 1, 2], [0, 2, 3], [0, 1, 3], [1, 2, 3], [4, 0, 1], [4, 1, 2], [4, 2, 3]]


def test_same_mesh_as_off_and_obj_parses_equal(tmp_path):
    verts, _ = mr.random_mesh(40, 5, -1e3, 1e3)
    rng = np.random.default_rng(6)
    polys = [tuple(int(i) for i in rng.integers(0, len(verts), int(k))) for k in rng.integers(3, 7, 30)]
    mr.write_off(tmp_path / 'a.off', verts, polys)
    mr.write_obj(tmp_path / 'a.obj', verts, polys)
    a, b = gd.read_mesh(str(tmp_path / 'a.off')), gd.read_mesh(str(tmp_path / 'a.obj'))
    assert np.array_equal(a[0].view(np.int64), verts.view(np.int64))          # repr() round-trips every double
    assert np.array_equal(a[0].view(np.int64), b[0].view(np.int64)) and np.array_equal(a[1], b[1])
    assert np.array_equal(a[1], mr.fan(polys))


def test_reader_errors_are_distinct(tmp_path):
    with pytest.raises(FileNotFoundError):
        gd.read_mesh(str(tmp_path / 'missing.off'))
    mr.write_off(tmp_path / 'cube.off', mr.CUBE_VERTS, mr.CUBE_QUADS)
    text = open(tmp_path / 'cube.off').read()
    (tmp_path / 'cut.off').write_text(text[:text.rindex('4 1 3')])          # the last face is missing
    with pytest.raises(gd.MeshFormatError):
        gd.read_mesh(str(tmp_path / 'cut.off'))
    (tmp_path / 'cut2.off').write_text('\n'.join(text.split('\n')[:6]) + '\n1.0 0.5')          # ends inside a vertex
    with pytest.raises(gd.MeshFormatError):
        gd.read_mesh(str(tmp_path / 'cut2.off'))
    (tmp_path / 'noise.off').write_text('ply\nformat ascii 1.0\n')
    with pytest.raises(gd.MeshFormatError):
        gd.read_mesh(str(tmp_path / 'noise.off'))
    (tmp_path / 'bad.obj').write_text('v 0 0 0\nv 1 0 0\nf 1 2 x\n')
    with pytest.raises(gd.MeshFormatError):
        gd.read_mesh(str(tmp_path / 'bad.obj'))
    (tmp_path / 'range.off').write_text(text.replace('4 1 3 7 5', '4 1 3 8 5'))
    with pytest.raises(gd.MeshIndexError):
        gd.read_mesh(str(tmp_path / 'range.off'))
    for face in ('f 1 2 4', 'f 1 2 0', 'f 1 2 -4'):
        (tmp_path / 'range.obj').write_text('v 0 0 0\nv 1 0 0\nv 0 1 0\n' + face + '\n')
        with pytest.raises(gd.MeshIndexError):
            gd.read_mesh(str(tmp_path / 'range.obj'))
    assert not issubclass(gd.MeshFormatError, gd.MeshIndexError) and not issubclass(gd.MeshIndexError, gd.MeshFormatError)
    assert issubclass(gd.MeshFormatError, PcgcError) and issubclass(gd.MeshIndexError, PcgcError)


def test_reference_function_surface():
    want = {'sample_points': ['mesh_filedir', 'n_points', 'resolution'], 'get_rotate_matrix': [],
            'mesh2pc': ['mesh_filedir', 'n_points', 'resolution'],
            'generate_dataset': ['mesh_filedirs', 'pc_rootdir', 'out_filetype', 'n_points', 'resolution'],
            'traverse_path_recursively': ['rootdir']}
    for name, lead in want.items():
        params = list(inspect.signature(getattr(gd, name)).parameters.values())
        assert [p.name for p in params[:len(lead)]] == lead, name
        for p in params[len(lead):]:                      # every extension is keyword-only or optional
            assert p.kind is p.KEYWORD_ONLY or p.default is not p.empty, (name, p.name)
    sig = inspect.signature(gd.generate_dataset).parameters
    assert sig['n_points'].default == 4e5 and sig['resolution'].default == 255
    assert sig['seed'].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(gd.mesh2pc).parameters
    assert sig['seed'].kind is inspect.Parameter.KEYWORD_ONLY and sig['rotation'].kind is inspect.Parameter.KEYWORD_ONLY
    sig = inspect.signature(gd.sample_points).parameters
    assert sig['n_points'].default == 4e5 and sig['resolution'].default == 255


def test_h5_raises_naming_h5py(tmp_path):
    with pytest.raises(ValueError, match='h5py'):
        gd.generate_dataset([], str(tmp_path), 'h5')


def test_rotation_matrix_is_orthogonal_and_seeded():
    a, b = gd.get_rotate_matrix(np.random.default_rng(3)), gd.get_rotate_matrix(np.random.default_rng(3))
    assert a.dtype == np.float64 and a.shape == (3, 3) and np.array_equal(a, b)
    assert np.allclose(a @ a.T, np.eye(3), atol=1e-12)
    assert gd.get_rotate_matrix().shape == (3, 3)


def test_traverse_and_argument_checks(tmp_path):
    (tmp_path / 'a' / 'b').mkdir(parents=True)
    for f in ('x.off', 'a/y.obj', 'a/b/z.txt'):
        (tmp_path / f).write_text('')
    got = sorted(gd.traverse_path_recursively(str(tmp_path)))
    assert got == sorted(str(tmp_path / f) for f in ('x.off', 'a/y.obj', 'a/b/z.txt'))
    for bad in (0, 1024):
        with pytest.raises(ValueError):
            gd.mesh2pc(str(tmp_path / 'x.off'), 100, bad)
    with pytest.raises(ValueError):
        gd.mesh2pc(str(tmp_path / 'x.off'), 0, 127)


def test_native_reader_counts_then_fills(tmp_path):
    from pcgcv2_amd._lib import lib
    p = tmp_path / 'cube.obj'
    mr.write_obj(p, mr.CUBE_VERTS, mr.CUBE_QUADS)
    counts = np.zeros(2, dtype=np.int64)
    assert lib().pcgc_mesh_read(str(p).encode(), None, 0, None, 0, counts.ctypes.data) == 0 and counts.tolist() == [8, 12]
    verts, faces = np.zeros((8, 3)), np.zeros((12, 3), dtype=np.int32)
    assert lib().pcgc_mesh_read(str(p).encode(), verts.ctypes.data, 8, faces.ctypes.data, 11, counts.ctypes.data) == -5      # too small
    assert not faces.any() and counts.tolist() == [8, 12]
    assert lib().pcgc_mesh_read(str(p).encode(), verts.ctypes.data, 8, faces.ctypes.data, 12, counts.ctypes.data) == 0
    assert np.array_equal(verts, mr.CUBE_VERTS) and np.array_equal(faces, mr.fan(mr.CUBE_QUADS))
