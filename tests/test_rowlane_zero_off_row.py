"""RL_F_ZERO_OFF_ROW of the model headers (symbolic/emit_rowlane.py::f_zero_off_row): whether every class body gives
f == 0 exactly, through finite intermediates, when all its state and parameter operands are 0.  Where it is true the
row-group kernels hand all-zero operands to the lanes that evaluate no row and drop the select that zeroed their f
(csrc/sbm_kernels_rowgroup.hpp, RowGroupSystem::kZeroOffRow); where it is false nothing changes.  No GPU needed.

The emitter decides on the expressions it prints, in exact arithmetic; the last test evaluates the classes' f in Python
floats at zeros instead (a reciprocal of 0 raises ZeroDivisionError there, 0/0 too) and asks for the same answer."""
import math
import re
from collections import OrderedDict

import pytest
import sympy


def _flag(src):
    m = re.search(r'static constexpr bool RL_F_ZERO_OFF_ROW = (true|false);', src)
    assert m, "RL_F_ZERO_OFF_ROW not printed"
    return m.group(1) == 'true'


def _emit(spec):
    from sysbio_modeling_amd.symbolic.emit import emit_hip, Derived
    d = Derived(spec)
    return emit_hip(spec, d), d


def test_true_for_the_cascade():
    from sysbio_modeling_amd import models_zoo
    src, _ = _emit(models_zoo.cascade_spec())                 # 0 * (0 * rcp(1)) - 0 * 0
    assert _flag(src)


def test_false_with_a_constant_production_term():
    from sysbio_modeling_amd.symbolic.emit import ModelSpec
    x0, x1, d0, d1 = sympy.symbols('x0 x1 d0 d1')
    spec = ModelSpec(name='const2', variables=['x0', 'x1'], params=['d0', 'd1'],
                     equations=OrderedDict([('x0', 0.5 - d0 * x0), ('x1', 0.25 - d1 * x1)]))      # f = k0 - d y
    src, _ = _emit(spec)
    assert not _flag(src)


def test_false_where_a_class_body_divides_by_a_state():
    from sysbio_modeling_amd.symbolic.emit import ModelSpec
    x0, x1, a, b = sympy.symbols('x0 x1 a b')
    spec = ModelSpec(name='recip2', variables=['x0', 'x1'], params=['a', 'b'],
                     equations=OrderedDict([('x0', a / x0 - b * x0), ('x1', a * x0 - b * x1)]))   # 1 / y
    src, _ = _emit(spec)
    assert not _flag(src)


def _numeric_zero(classes):
    """every class's f evaluated in Python floats with all operands 0.0: finite and equal to 0"""
    for c in classes:
        f = c['canon'][0]
        syms = sorted(f.free_symbols, key=str)
        if any(not s.name.startswith(('YS_', 'PS_')) for s in syms):
            return False                                                 # (depends on t: no statement about all t)
        fn = sympy.lambdify(syms, f, modules=[{'SBM_RCP': lambda v: 1.0 / v}, 'math'])
        try:
            v = fn(*[0.0] * len(syms))
        except (ZeroDivisionError, ValueError, OverflowError):
            return False
        if not (math.isfinite(v) and v == 0.0):
            return False
    return True


@pytest.mark.parametrize('name', ['simple', 'michaelis_menten', 'cascade20', 'stiff50'])
def test_committed_header_agrees_with_a_numeric_evaluation(name):
    from sysbio_modeling_amd.symbolic import ZOO_NAMES, zoo_model
    from sysbio_modeling_amd.symbolic import emit_rowlane
    assert set(ZOO_NAMES) == {'simple', 'michaelis_menten', 'cascade20', 'stiff50'}
    gm = zoo_model(name)
    classes, _ = emit_rowlane.find_classes(gm.spec, gm.derived)
    numeric = _numeric_zero(classes)
    print(name, 'header', _flag(gm.hip_source), 'numeric', numeric)
    assert _flag(gm.hip_source) == numeric
