"""DeviceTarget and flow.target_vectors on the CPU: a target's vectors are staged once per device, pass through the bindings'
staging untouched, and are never reused under another transform."""
import numpy as np
import pytest
import torch


def test_staged_once_and_never_under_another_transform():
    from nnest_amd import flow
    from nnest_amd.device_target import DeviceTarget
    t = DeviceTarget(3, (0.5,), np.array([2.0, 4.0]), np.array([1.0, -1.0]), [-5, -5], [5, 5])
    kw, again = t.launch_kwargs('cpu'), t.launch_kwargs(torch.device('cpu'))
    assert set(kw) == {'t_std', 't_mean', 'lo', 'hi', 'like_params'} and kw['like_params'] == (0.5,) and t.like_id == 3
    for k in ('t_std', 't_mean', 'lo', 'hi'):
        assert again[k] is kw[k] and kw[k].dtype == torch.float32 and kw[k].shape == (2,)
    np.testing.assert_array_equal(t.transform(torch.tensor([[1.0, 2.0]])).numpy(), [[3.0, 7.0]])
    # the bindings' staging hands such tensors on as they are
    assert all(a is kw[k] for a, k in zip(flow.target_vectors('t', 'cpu', kw['t_std'], kw['t_mean'], kw['lo'], kw['hi'], D=2),
                                          ('t_std', 't_mean', 'lo', 'hi')))
    # the fields are fixed; another T is another target with its own tensors, the same likelihood and box
    with pytest.raises(AttributeError, match='with_transform'):
        t.t_std = np.ones(2)
    with pytest.raises(ValueError):
        t.t_mean[0] = 3.0
    u = t.with_transform([1.0, 0.5], [0.0, 2.0])
    ukw = u.launch_kwargs('cpu')
    assert ukw['t_std'] is not kw['t_std'] and (u.like_id, u.like_params) == (3, (0.5,))
    np.testing.assert_array_equal(ukw['t_std'].numpy(), [1.0, 0.5])
    np.testing.assert_array_equal(ukw['lo'].numpy(), [-5.0, -5.0])
    np.testing.assert_array_equal(t.launch_kwargs('cpu')['t_std'].numpy(), [2.0, 4.0])
    # no T and no box
    bare = DeviceTarget(0)
    assert bare.launch_kwargs('cpu') == dict(t_std=None, t_mean=None, lo=None, hi=None, like_params=())
    x = torch.ones(1, 2)
    assert bare.transform(x) is x


def test_target_vectors_pairs_and_identity():
    from nnest_amd import flow
    from nnest_amd.device_target import DeviceTarget
    for bad in (dict(t_std=[1.0]), dict(t_mean=[1.0]), dict(lo=[1.0]), dict(hi=[1.0])):
        args = dict(dict(t_std=None, t_mean=None, lo=None, hi=None), **bad)
        with pytest.raises(ValueError, match='both or neither'):
            flow.target_vectors('who', 'cpu', D=1, **args)
        with pytest.raises(ValueError, match='both or neither'):
            DeviceTarget(0, (), **bad)
    assert flow.target_vectors('who', 'cpu', None, None, None, None, D=3) == (None, None, None, None)
    std, mean, lo, hi = flow.target_vectors('who', 'cpu', None, None, None, None, D=3, identity=True)
    assert std.tolist() == [1.0] * 3 and mean.tolist() == [0.0] * 3 and lo is None and hi is None
    with pytest.raises(Exception):   # a vector that is not [D]
        flow.target_vectors('who', 'cpu', [1.0, 2.0], [0.0, 0.0], None, None, D=3)
