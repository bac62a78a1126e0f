"""`.r1cs` reader (iden3 binary format v1) -- thin wrapper over the native reader of libdg16
(`dg16_r1cs_parse`, csrc/formats.hip), the counterpart of the reference's `R1CSFile::new` / `R1CS::from`
(ark-circom/src/circom/r1cs_reader.rs:54-249, r1cs.rs): header checks, constraint section -> CSR arrays the GPU
kernel `dg16_qap` consumes, wire map.

Same error behaviour as the reference: bad magic, version != 1, field size != 32 bytes and a prime other
than the BN254 scalar modulus are rejected (r1cs_reader.rs:58-72,161-188)."""

import ctypes

import numpy as np

from . import lib as _lib

BN254_R_LE = bytes.fromhex("010000f093f5e1439170b97948e833285d588181b64550b829a031e1724e6430")


class R1CSError(ValueError):
    pass


class R1CS:
    """num_inputs counts the constant 1 (arkworks' instance variable 0), like `R1CS::from`."""

    def __init__(self, data: bytes):
        L = _lib.load()
        data = bytes(data)
        h = ctypes.c_void_p()
        if L.dg16_r1cs_parse(data, len(data), ctypes.byref(h)) != 0:
            raise R1CSError(L.dg16_io_error().decode())
        try:
            hd = _lib.R1csHeader()
            L.dg16_r1cs_header_get(h, ctypes.byref(hd))
            self.n_wires, self.n_pub_out, self.n_pub_in = hd.n_wires, hd.n_pub_out, hd.n_pub_in
            self.n_prv_in, self.n_labels, self.n_constraints = hd.n_prv_in, hd.n_labels, hd.n_constraints
            self.num_inputs = 1 + self.n_pub_in + self.n_pub_out
            self.num_variables = self.n_wires
            self.num_aux = self.n_wires - self.num_inputs
            self.csr = []
            for k in range(3):
                m = _lib.Csr()
                L.dg16_r1cs_matrix(h, k, ctypes.byref(m))
                self.csr.append(m.arrays())
            self.wire_mapping = None
            if hd.has_wire_map:
                p = ctypes.POINTER(ctypes.c_uint64)()
                L.dg16_r1cs_wire_map(h, ctypes.byref(p))
                self.wire_mapping = np.ctypeslib.as_array(p, shape=(self.n_wires,)).copy()
        finally:
            L.dg16_r1cs_free(h)

    @classmethod
    def from_file(cls, path):
        import lzma
        raw = open(path, "rb").read()
        if path.endswith(".xz"):
            raw = lzma.decompress(raw)
        return cls(raw)

    def rows(self, k):
        """Matrix k (0 = A, 1 = B, 2 = C) as a list of [(coeff_int, index)] rows (canonical integers)."""
        row_ptr, col, coeff = self.csr[k]
        ints = [int.from_bytes(coeff[i].tobytes(), "little") for i in range(coeff.shape[0])]
        return [[(ints[j], int(col[j])) for j in range(row_ptr[i], row_ptr[i + 1])]
                for i in range(self.n_constraints)]


def check_witness(ctx, curve, r1cs, assignment):
    """Is `assignment` (the full assignment [1, public.., witness..] as integers, or a uint64 [n][4] array of canonical
    values) a satisfying one?  Runs dg16_qap_r1cs on the GPU -- the evaluation pass a Libsnark proof starts with, whose
    fused check compares a_i b_i with c_i on every constraint row -- and returns (n_violated, first_row | None).
    r1cs: an R1CS (canonical coefficients) or a dict with num_constraints, num_inputs, a / b / c = (row_ptr, col,
    coeff) and coeff_mont (default True: coefficients already in Montgomery form)."""
    if isinstance(r1cs, dict):
        nc, ni = int(r1cs["num_constraints"]), int(r1cs["num_inputs"])
        csr = [r1cs["a"], r1cs["b"], r1cs["c"]]
        coeff_mont = bool(r1cs.get("coeff_mont", True))
    else:
        nc, ni, csr, coeff_mont = int(r1cs.n_constraints), int(r1cs.num_inputs), list(r1cs.csr), False
    if isinstance(assignment, np.ndarray):
        w = np.ascontiguousarray(assignment, dtype=np.uint64).reshape(-1, 4)
    else:
        w = np.array([[(int(x) >> (64 * j)) & (2**64 - 1) for j in range(4)] for x in assignment], dtype=np.uint64)
    mats = []
    for ptr, col, coeff in csr:
        coeff = np.ascontiguousarray(coeff, dtype=np.uint64).reshape(-1, 4)
        if not coeff_mont and coeff.shape[0]:
            coeff = ctx.field_op(curve, "fr", "to_mont", coeff)
        mats.append((np.ascontiguousarray(ptr, dtype=np.uint32), np.ascontiguousarray(col, dtype=np.uint32), coeff))
    return ctx.qap_r1cs(curve, nc, ni, mats[0], mats[1], mats[2], w, scalars_mont=False)[3]
