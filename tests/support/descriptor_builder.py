"""TEST INFRASTRUCTURE -- hand-built ``sbm_project_desc`` descriptors (include/sbm.h) for tests that need shapes no
Project of the zoo has: any parameter map, any grid lengths, rows in any order, any mix of 'direct' / 'sum' / custom
rows, programs written opcode by opcode.  ``Descriptor`` holds the arrays, ``LoadedProject`` loads them through
sbm_project_load and calls sbm_jacobian_batch; ``sample_inputs`` integrates every experiment on its own grid through
sbm_sens_batch_host, the inputs of the wide reference (tests/support/assembly_reference.map_reference).
Also here: the custom programs of the opcode tests and the running error bound of a program."""
from __future__ import annotations

import ctypes
import math

import numpy as np

U = 2.0 ** -53
_i32 = lambda a: np.ascontiguousarray(a, dtype=np.int32)
_f64 = lambda a: np.ascontiguousarray(a, dtype=np.float64)


# ------------------------------------------------------------------------------------------------------------------
# programs
# ------------------------------------------------------------------------------------------------------------------
def _op():
    from sysbio_modeling_amd.project.observables import OP
    return OP


def walk_program(code):
    """(opcode, inline operand or None) per instruction, END included"""
    OP = _op()
    out, pc = [], 0
    while pc < len(code):
        op = int(code[pc])
        if op in (OP['VAR'], OP['CONST'], OP['POWI']):
            out.append((op, int(code[pc + 1])))
            pc += 1
        else:
            out.append((op, None))
        pc += 1
    return out


def program_depth(code):
    OP = _op()
    depth = worst = 0
    for op, _ in walk_program(code):
        if op in (OP['VAR'], OP['CONST'], OP['TIME']):
            depth += 1
        elif op in (OP['ADD'], OP['SUB'], OP['MUL'], OP['DIV'], OP['POW']):
            depth -= 1
        worst = max(worst, depth)
    return worst


# the model variables of the opcode tests: the 20 states of cascade20
OPCODE_VARIABLES = ['x%d' % i for i in range(20)]
# what compile_observable turns these into uses ADD MUL NEG POW POWI EXP LOG SQRT TANH SIN COS ABS SIGN TIME VAR CONST
# (a - b compiles to NEG ADD and a / b to POWI -1 MUL: SUB, DIV and POWI 0 / 1 come from the hand-written program below)
OPCODE_PROGRAMS = {
    'ratio': 'x4 / (x4 + x9)',
    'powers': 'x1**2 + 0.001 * x3**(-3) + (x2 / 4)**64 + 1 / x5',
    'pow_frac': 'x1**2.5 * tanh(x3) - log(x1) + exp(-x2)',
    'trig_time': 'sin(x6) * cos(t / 7) + sqrt(x7) * t',
    'abs_sign': 'abs(x2 - 1.0) + abs(x0) * x2 + abs(x0 - 2.5)',
}
ZERO_SAFE_PROGRAMS = ('abs_sign',)       # may be sampled where every state is exactly 0 (index 0 of a grid from t0 = 0)
HOST_LIBM_ULP = dict(EXP=1.0, LOG=1.0, TANH=2.0, SIN=1.0, COS=1.0, POW=1.0)     # glibc's documented double-precision errors


def hand_program(kind, n=16):
    """Programs written opcode by opcode, in compile_observable's output format, with the sympy expression they state.
    'sub_div_powi': (x0 - x1) / x1 + x0^1 + x1^0   -- SUB, DIV, POWI 1, POWI 0
    'deep':         x0 + x0 + ... (n pushes, then n - 1 ADDs): a stack n deep"""
    import sympy
    OP = _op()
    x0, x1 = sympy.Symbol('__obs_y0', real=True), sympy.Symbol('__obs_y1', real=True)
    if kind == 'sub_div_powi':
        g = [OP['VAR'], 0, OP['VAR'], 1, OP['SUB'], OP['VAR'], 1, OP['DIV'], OP['VAR'], 0, OP['POWI'], 1, OP['ADD'],
             OP['VAR'], 1, OP['POWI'], 0, OP['ADD'], OP['END']]
        d0 = [OP['CONST'], 0, OP['VAR'], 1, OP['DIV'], OP['CONST'], 0, OP['ADD'], OP['END']]
        d1 = [OP['VAR'], 0, OP['NEG'], OP['VAR'], 1, OP['POWI'], 2, OP['DIV'], OP['END']]
        return dict(variables=[0, 1], subprograms=[g, d0, d1], constants=[1.0], expr=(x0 - x1) / x1 + x0 + 1, symbols=[x0, x1])
    if kind == 'deep':
        g = [OP['VAR'], 0] * n + [OP['ADD']] * (n - 1) + [OP['END']]
        return dict(variables=[0], subprograms=[g, [OP['CONST'], 0, OP['END']]], constants=[float(n)], expr=n * x0, symbols=[x0])
    raise ValueError(kind)


HAND_POWI_PROGRAM = None       # set below (needs OP): the value subprogram of 'sub_div_powi'


def deep_program(n):
    return hand_program('deep', n)['subprograms'][0]


def _init_hand():
    global HAND_POWI_PROGRAM
    HAND_POWI_PROGRAM = hand_program('sub_div_powi')['subprograms'][0]


_init_hand()


def all_test_programs():
    """{name: program} of everything the opcode tests load: the compiled expressions and the hand-written programs"""
    from sysbio_modeling_amd.project.observables import compile_observable
    out = {nm: compile_observable(text, OPCODE_VARIABLES) for nm, text in OPCODE_PROGRAMS.items()}
    out['sub_div_powi'] = hand_program('sub_div_powi')
    out['deep16'] = hand_program('deep', 16)
    return out


TEST_PROGRAM_NAMES = sorted(OPCODE_PROGRAMS) + ['deep16', 'sub_div_powi']


def program_error_bound(code, consts, values, t, libm_ulp):
    """Absolute bound on the float64 result of a program: half an ulp (u |result|) per arithmetic operation and per
    multiplication of POWI, ``libm_ulp[f]`` ulps (2 u |result| each) per library function, every operand's error carried
    to first order through the operation's derivative -- summed along the program.  Inputs are exact.  A SIGN whose
    argument cannot be told from zero gives inf."""
    OP = _op()
    name = {v: k for k, v in OP.items()}
    st = []          # (value, error bound)
    for op, arg in walk_program(code):
        nm = name[op]
        if nm == 'END':
            break
        if nm == 'VAR':
            st.append((float(values[arg]), 0.0))
        elif nm == 'CONST':
            st.append((float(consts[arg]), 0.0))
        elif nm == 'TIME':
            st.append((float(t), 0.0))
        elif nm in ('ADD', 'SUB', 'MUL', 'DIV', 'POW'):
            (b, eb), (a, ea) = st.pop(), st.pop()
            with np.errstate(all='ignore'):
                if nm == 'ADD':
                    r, e = a + b, ea + eb
                elif nm == 'SUB':
                    r, e = a - b, ea + eb
                elif nm == 'MUL':
                    r, e = a * b, abs(a) * eb + abs(b) * ea
                elif nm == 'DIV':
                    r = a / b if b != 0 else math.inf
                    e = ea / abs(b) + abs(a) * eb / (b * b) if b != 0 else math.inf
                else:
                    r = math.pow(a, b)
                    e = abs(b * math.pow(a, b - 1.0)) * ea + (abs(r * math.log(a)) * eb if eb else 0.0)
                    e += 2.0 * libm_ulp['POW'] * U * abs(r) - U * abs(r)
            st.append((r, e + U * abs(r)))
        elif nm == 'POWI':
            a, ea = st.pop()
            n = abs(arg)
            r = a ** n if n else 1.0
            e = n * abs(a) ** (n - 1) * ea if n else 0.0
            mults = 2 * max(n.bit_length(), 1) if n > 1 else 0
            e += mults * U * abs(r)
            if arg < 0:
                e = e / (r * r) + U / abs(r)
                r = 1.0 / r
            st.append((r, e))
        else:
            a, ea = st.pop()
            if nm == 'NEG':
                st.append((-a, ea))
            elif nm == 'ABS':
                st.append((abs(a), ea))
            elif nm == 'SIGN':
                st.append((float((a > 0) - (a < 0)), 0.0 if abs(a) > ea or (a == 0.0 and ea == 0.0) else math.inf))
            elif nm == 'SQRT':
                r = math.sqrt(a)
                st.append((r, (ea / (2.0 * r) if ea else 0.0) + U * r))
            else:
                f = {'EXP': math.exp, 'LOG': math.log, 'TANH': math.tanh, 'SIN': math.sin, 'COS': math.cos}[nm]
                r = f(a)
                d = {'EXP': abs(r), 'LOG': 1.0 / abs(a), 'TANH': 1.0 - r * r, 'SIN': abs(math.cos(a)), 'COS': abs(math.sin(a))}[nm]
                st.append((r, d * ea + 2.0 * libm_ulp[nm] * U * abs(r)))
    assert len(st) == 1
    return st[0][1]


# ------------------------------------------------------------------------------------------------------------------
# descriptors
# ------------------------------------------------------------------------------------------------------------------
class Descriptor(object):
    """rows: dicts with exp, tidx, vars (model variable indices), data, sigma, sf (group or -1) and, for a custom row,
    prog (a key of ``programs``; its variables replace ``vars``).  programs: {name: compile_observable(...) or
    hand_program(...)}.  grids: one increasing array of output times per experiment.  pmap / pfixed [E][NP]."""

    def __init__(self, n_vars, sens_col, q, pmap, pfixed, grids, rows, n_groups=0, programs=None, prior=None, sf_prior=None,
                 compat=0, loss=0, var_names=None):
        from sysbio_modeling_amd.project.observables import program_tables
        self.n_vars, self.q, self.G, self.compat, self.loss = int(n_vars), int(q), int(n_groups), int(compat), int(loss)
        self.sens_col = _i32(sens_col)
        self.NP = len(self.sens_col)
        self.pmap, self.pfixed = _i32(pmap).reshape(-1, self.NP), _f64(pfixed).reshape(-1, self.NP)
        self.E = self.pmap.shape[0]
        self.grids = [np.asarray(g, dtype=float) for g in grids]
        assert len(self.grids) == self.E
        self.tgrid_off = _i32(np.concatenate([[0], np.cumsum([len(g) for g in self.grids])]))
        self.tgrid = _f64(np.concatenate(self.grids))
        self.n_t_max = max(len(g) for g in self.grids)
        programs = programs or {}
        self.programs = programs
        self.rows = rows
        R = self.R = len(rows)
        var_off, var_list, measures = [0], [], []
        for r in rows:
            vs = programs[r['prog']]['variables'] if r.get('prog') is not None else list(r['vars'])
            var_list.extend(int(v) for v in vs)
            var_off.append(len(var_list))
            measures.append(r['prog'] if r.get('prog') is not None else '~plain')
        self.row_exp, self.row_tidx = _i32([r['exp'] for r in rows]), _i32([r['tidx'] for r in rows])
        self.row_var_off, self.row_vars = _i32(var_off), _i32(var_list if var_list else [0])
        self.row_data, self.row_sigma = _f64([r['data'] for r in rows]), _f64([r['sigma'] for r in rows])
        self.row_sf = _i32([r.get('sf', -1) for r in rows])
        self.row_time = _f64([r.get('time', self.grids[r['exp']][r['tidx']]) for r in rows])
        self.tables = program_tables(measures, programs) if programs else None
        self.prior = prior if prior is not None else (_i32([]), _f64([]), _f64([]))
        self.sf_prior = sf_prior if sf_prior is not None else (_i32([]), _f64([]), _f64([]))
        self.prior = (_i32(self.prior[0]), _f64(self.prior[1]), _f64(self.prior[2]))
        self.sf_prior = (_i32(self.sf_prior[0]), _f64(self.sf_prior[1]), _f64(self.sf_prior[2]))
        self.row_expr = [(programs[r['prog']]['expr'], programs[r['prog']]['symbols']) if r.get('prog') is not None else None
                         for r in rows]

    def reference_arrays(self):
        """what assembly_reference.map_reference reads"""
        return dict(n_rows=self.R, n_project_params=self.q, sens_col=self.sens_col, pmap=self.pmap, row_exp=self.row_exp,
                    row_tidx=self.row_tidx, row_var_off=self.row_var_off, row_vars=self.row_vars, row_time=self.row_time,
                    row_expr=self.row_expr if self.programs else None)

    def ctypes_desc(self):
        from sysbio_modeling_amd import _lib
        nil_i, nil_d = ctypes.cast(None, _lib.c_int32_p), ctypes.cast(None, _lib.c_double_p)
        ip = lambda x: x.ctypes.data_as(_lib.c_int32_p) if x.size else nil_i
        dp = lambda x: x.ctypes.data_as(_lib.c_double_p) if x.size else nil_d
        t = self.tables
        prog = (t['n_programs'], len(t['prog_code']), len(t['prog_const']), ip(t['row_prog']), ip(t['prog_nvars']),
                ip(t['prog_sub_off']), ip(t['prog_code']), dp(t['prog_const']), dp(self.row_time)) if t else \
            (0, 0, 0, nil_i, nil_i, nil_i, nil_i, nil_d, nil_d)
        return _lib.ProjectDesc(self.E, self.q, self.R, self.G, len(self.prior[0]), len(self.sf_prior[0]),
                                ip(self.pmap), dp(self.pfixed), ip(self.sens_col), ip(self.tgrid_off), dp(self.tgrid),
                                ip(self.row_exp), ip(self.row_tidx), ip(self.row_var_off), ip(self.row_vars),
                                dp(self.row_data), dp(self.row_sigma), ip(self.row_sf),
                                ip(self.prior[0]), dp(self.prior[1]), dp(self.prior[2]),
                                ip(self.sf_prior[0]), dp(self.sf_prior[1]), dp(self.sf_prior[2]), self.compat, self.loss, *prog)


def try_load(model, desc):
    """(rc, handle, message) of sbm_project_load; ``model``: an OdeModel on the device"""
    from sysbio_modeling_amd import _lib
    lib = _lib.load_library()
    h = ctypes.c_void_p()
    d = desc.ctypes_desc()
    rc = lib.sbm_project_load(model.device_model.handle, ctypes.byref(d), ctypes.byref(h))
    msg = lib.sbm_last_error()
    return rc, h, (msg.decode() if msg else '')


class LoadedProject(object):
    def __init__(self, model, desc):
        from sysbio_modeling_amd import _lib
        self.lib, self.model, self.desc = _lib.load_library(), model, desc
        rc, self.handle, msg = try_load(model, desc)
        if rc != 0:
            raise _lib.SbmError("sbm_project_load failed (%d): %s" % (rc, msg))

    def close(self):
        if self.handle:
            self.lib.sbm_project_unload(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def jacobian(self, theta, opts, fill=7.0):
        """every output of sbm_jacobian_batch (and the per-trajectory step counts) as numpy arrays; buffers are
        prefilled so that an entry the kernel does not write shows"""
        import torch
        from sysbio_modeling_amd import _lib
        d = self.desc
        theta = np.ascontiguousarray(theta, dtype=np.float64).reshape(-1, d.q)
        V = theta.shape[0]
        RT = d.R + len(d.prior[0]) + len(d.sf_prior[0])
        dev = lambda *shape: torch.full(shape, fill, dtype=torch.float64, device='cuda')
        idev = lambda *shape: torch.full(shape, -7, dtype=torch.int32, device='cuda')
        th = torch.from_numpy(theta).cuda()
        out = dict(sims=dev(V, d.R), R_out=dev(V, RT), J=dev(V, RT, d.q), Jmodel=dev(V, d.R, d.q), sf=dev(V, max(d.G, 1)),
                   sf_grad=dev(V, max(d.G, 1), d.q), norms=dev(V), grad=dev(V, d.q), status=idev(V), n_steps=idev(V))
        p = _lib.dev_ptr
        rc = self.lib.sbm_jacobian_batch(self.handle, p(th), V, ctypes.byref(opts), p(out['sims']), p(out['R_out']), p(out['J']),
                                         p(out['Jmodel']), p(out['sf']), p(out['sf_grad']), p(out['norms']), p(out['grad']),
                                         p(out['status']), p(out['n_steps']))
        _lib.check(rc, 'sbm_jacobian_batch')
        steps = idev(V, d.E)
        _lib.check(self.lib.sbm_project_trajectory_steps(self.handle, V, p(steps)), 'sbm_project_trajectory_steps')
        torch.cuda.synchronize()
        res = {k: v.cpu().numpy() for k, v in out.items()}
        res['sf'], res['sf_grad'] = res['sf'][:, :d.G], res['sf_grad'][:, :d.G]
        res['traj_steps'] = steps.cpu().numpy()
        return res


def experiment_parameters(desc, theta, shift=0):
    """P [V][E][NP] = exp(theta[pmap]) or pfixed, gathered on the host; shift = -1 / +1 moves every MAPPED parameter one
    ulp down / up (the device computes exp itself: its P may differ from numpy's in the last bit)"""
    theta = np.asarray(theta, dtype=np.float64).reshape(-1, desc.q)
    mapped = desc.pmap >= 0
    with np.errstate(over='ignore'):
        P = np.where(mapped[None], np.exp(theta[:, np.where(mapped, desc.pmap, 0)]), desc.pfixed[None])
    if shift:
        P = np.where(mapped[None], np.nextafter(P, np.inf if shift > 0 else -np.inf), P)
    return P


def sample_inputs(model, desc, theta, opts, shift=0):
    """Y [V][E][n_t_max][NV], S [V][E][n_t_max][NV][NK] (padding NaN): sbm_sens_batch_host per experiment on that
    experiment's grid (experiments with the same grid share a call: one trajectory per wavefront either way)."""
    P = experiment_parameters(desc, theta, shift)
    V = P.shape[0]
    dm = model.device_model
    Y = np.full((V, desc.E, desc.n_t_max, dm.n_vars), np.nan)
    S = np.full((V, desc.E, desc.n_t_max, dm.n_vars, dm.n_sens), np.nan)
    by_grid = {}
    for e, g in enumerate(desc.grids):
        by_grid.setdefault(g.tobytes(), []).append(e)
    for key, exps in by_grid.items():
        g = desc.grids[exps[0]]
        y, s, st, _, _ = dm.sens_host(P[:, exps].reshape(V * len(exps), -1), g, None, opts)
        Y[:, exps, :len(g)] = y.reshape(V, len(exps), len(g), dm.n_vars)
        S[:, exps, :len(g)] = s.reshape(V, len(exps), len(g), dm.n_vars, dm.n_sens)
    return Y, S
