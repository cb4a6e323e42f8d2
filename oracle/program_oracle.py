"""ORACLE (test infrastructure, not product code): the stack machine that evaluates compiled 'custom' observables in
the assembly kernel (csrc/sbm_observable_program.hpp::sbm_prog_eval, opcodes of include/sbm.h), restated in Python so that the
compiler (sysbio_modeling_amd/project/observables.py) can be checked without a GPU.
Only tests/ may import this."""
import math

OPS = ['END', 'VAR', 'CONST', 'ADD', 'SUB', 'MUL', 'DIV', 'NEG', 'POW', 'POWI', 'EXP', 'LOG', 'SQRT', 'TANH', 'SIN',
       'COS', 'ABS', 'SIGN', 'TIME']


def run(code, consts, values, t=0.0):
    """values[k] = value of the k-th listed variable."""
    st, pc = [], 0
    while True:
        op = OPS[code[pc]]
        if op == 'END':
            break
        if op == 'VAR':
            pc += 1
            st.append(float(values[code[pc]]))
        elif op == 'CONST':
            pc += 1
            st.append(float(consts[code[pc]]))
        elif op == 'TIME':
            st.append(float(t))
        elif op in ('ADD', 'SUB', 'MUL', 'DIV', 'POW'):
            b = st.pop()
            a = st.pop()
            st.append({'ADD': a + b, 'SUB': a - b, 'MUL': a * b, 'DIV': a / b if op == 'DIV' else 0.0,
                       'POW': math.pow(a, b) if op == 'POW' else 0.0}[op])
        elif op == 'POWI':
            pc += 1
            st[-1] = st[-1] ** code[pc]
        else:
            x = st.pop()
            st.append({'NEG': lambda: -x, 'EXP': lambda: math.exp(x), 'LOG': lambda: math.log(x),
                       'SQRT': lambda: math.sqrt(x), 'TANH': lambda: math.tanh(x), 'SIN': lambda: math.sin(x),
                       'COS': lambda: math.cos(x), 'ABS': lambda: abs(x),
                       'SIGN': lambda: (x > 0) - (x < 0)}[op]())
        pc += 1
    assert len(st) == 1
    return st[0]
