// compute_msm.js -- the reference's entry point, kept intact, over the HIP engine.
//
//   export const compute_msm = async (bufferPoints, bufferScalars, log_result = true, force_recompile = false)
//       : Promise<{ x: bigint; y: bigint }>                       (submission/submission.ts:73-78)
//
// bufferPoints : Buffer of n x (x[32 B LE] || y[32 B LE]) canonical affine coordinates (README.md:297-299)
// bufferScalars: Buffer of n x 32 B LE scalars
// The BigIntPoint[] / bigint[] forms in the reference's type are converted with the harness's own
// encoder rule (bigIntsToBufferLE, reference/webgpu/utils.ts:90-99); U32ArrayPoint[] is, as in the
// reference (submission.ts:159-160 casts to Buffer), not supported.
'use strict';
const path = require('path');
const native = require(path.join(__dirname, 'te_msm_napi.node'));

const toLE32 = (v) => {
  const b = Buffer.alloc(32);
  let t = BigInt(v);
  for (let i = 0; i < 32; i++) { b[i] = Number(t & 0xffn); t >>= 8n; }
  return b;
};
const fromLE32 = (buf, off) =>          // four 64-bit words (a byte loop costs 64 BigInt operations per coordinate)
  buf.readBigUInt64LE(off) | (buf.readBigUInt64LE(off + 8) << 64n) | (buf.readBigUInt64LE(off + 16) << 128n) | (buf.readBigUInt64LE(off + 24) << 192n);

const asPointsBuffer = (p) => {
  if (Buffer.isBuffer(p)) return p;
  if (Array.isArray(p) && (p.length === 0 || typeof p[0].x === 'bigint')) {
    return Buffer.concat(p.map((q) => Buffer.concat([toLE32(q.x), toLE32(q.y)])));
  }
  throw new Error('compute_msm: bufferPoints must be a Buffer (or BigIntPoint[])');
};
const asScalarsBuffer = (s) => {
  if (Buffer.isBuffer(s)) return s;
  if (Array.isArray(s) && (s.length === 0 || typeof s[0] === 'bigint')) return Buffer.concat(s.map(toLE32));
  throw new Error('compute_msm: bufferScalars must be a Buffer (or bigint[])');
};

const compute_msm = async (bufferPoints, bufferScalars, log_result = true, force_recompile = false) => {
  // force_recompile exists to defeat WGSL pipeline caching (shader_manager.ts:85-92); the closest
  // meaning here is "drop cached engine state"
  if (force_recompile) native.resetContext();
  const out = await native.msmNative(asPointsBuffer(bufferPoints), asScalarsBuffer(bufferScalars));
  const result = { x: fromLE32(out, 0), y: fromLE32(out, 32) };
  if (log_result) console.log(result);
  return result;
};

// Not part of the reference's interface: which GPUs a call is sharded over (default TE_MSM_DEVICES, else device 0).
// Promises in flight at the same time overlap on the engine's work sets (js/addon.cc).
const setDevices = (ids) => native.setDevices(ids);
const getDevices = () => native.getDevices();
// Opt-in, also outside the reference's interface: setBases(bufferPoints) binds that Buffer once (upload + conversion on every
// device); compute_msm(bufferPoints, scalars) with THE SAME Buffer object then moves the scalars only.  The harness passes one
// point buffer to six calls per size (submission/miscellaneous/full_benchmarks.ts:63-68,100-105).  setBases(null) unbinds.
// setBases(bufferPoints, { montgomery: true }): the coordinates are a native prover's Montgomery residues (x * 2^256 mod p, what arkworks
// and snarkVM hold in memory); the bound set and every result over it are the same.
const setBases = (bufferPoints, options) => native.setBases(bufferPoints === undefined ? null : bufferPoints, options);
// Opt-in as well: setScalarsMontgomery(true) -- the scalar buffers of later compute_msm / msmBatch / msmIndexed calls hold Montgomery
// residues k * 2^256 mod L (L: the order of the prime subgroup), decoded on the GPU where the scalars are first read; any 256-bit value
// stands for its residue.  scalarMul / scalarMulX take canonical scalars only and throw while it is set.
const setScalarsMontgomery = (flag) => native.setScalarsMontgomery(!!flag);
// setScalarRecordBytes(n): the engine's option "scalar_record_bytes" for later calls (0 = the curve's own record; 32 and 48 spelled out).
// On the Twisted-Edwards curve the addon runs, 0 and 32 are the same thing and 48 makes every call that reads scalars reject.
// 8 / 16: the scalar buffers of compute_msm, msmBatch and msmIndexed are native u64 / u128 arrays (n * 8 / n * 16 bytes, little-endian).
const setScalarRecordBytes = (n) => native.setScalarRecordBytes(n);
// setScalarBits(b): the engine's option "scalar_bits" for later calls -- every scalar is below 2^b (0 = nothing declared): fewer windows.
const setScalarBits = (b) => native.setScalarBits(b);
const getStats = () => native.getStats();
// Opt-in as well: setCheckPoints(level) validates the input points of later calls (0 = none, default; 1 = canonical and on the
// curve; 2 = also in the prime-order subgroup, costly -- best paired with setBases, which then checks the set once).  A call with
// a bad point rejects with an Error naming the lowest failing index and the reason; setBases throws for a bad set.
const setCheckPoints = (level) => native.setCheckPoints(level);
// Outside the reference's interface: pointsFromX(xs) turns n x 32-byte little-endian x-coordinates (Aleo group values, what
// Address.msm takes) into the 64n-byte points buffer of compute_msm / setBases, y recovered on the GPU.  A bad x throws an Error
// naming the lowest failing index and the reason (also as .index / .reason).
const pointsFromX = (xs) => native.pointsFromX(xs);
// Outside the reference's interface too: scalarMul(points, scalars) returns the n points [k_i] P_i (no sum) as a 64n-byte Buffer;
// scalarMulX(xs, scalars) takes x-only points (bulkGroupScalarMul's counterpart).  One 32-byte scalar is shared by every point.  A
// bad point or x throws an Error naming the lowest failing index and the reason (also as .index / .reason).
const scalarMul = (points, scalars) => native.scalarMul(points, scalars);
const scalarMulX = (xs, scalars) => native.scalarMulX(xs, scalars);
// Fixed-base batch scalar multiplication: setBase(point) binds one 64-byte point (its table is built once, and again on a context that
// replaces the cached one); scalarMulBase(scalars) returns the n points [k_i] P as a 64n-byte Buffer -- scalarMul over the point
// replicated, without the doublings.  setScalarsMontgomery applies to these scalars.
const setBase = (point) => native.setBase(point);
const scalarMulBase = (scalars) => native.scalarMulBase(scalars);
// groupAdd(a, b, {subtract}) returns the n points A_i + B_i (A_i - B_i with subtract) as a 64n-byte Buffer, one 64-byte b shared by every
// a; groupAddX(ax, bx, {subtract}) takes x-only points (bulkAddGroups' counterpart).  groupSum(points) / groupSumX(xs) return the one
// point sum P_i as 64 bytes x || y (reduceGroups' counterpart; no points: (0, 1)).  A bad point (setCheckPoints) or a bad x throws an
// Error with .index, .reason and .operand (0 = a or the sum's input, 1 = b).
const groupAdd = (a, b, opts) => native.groupAdd(a, b, opts);
const groupAddX = (ax, bx, opts) => native.groupAddX(ax, bx, opts);
const groupSum = (points) => native.groupSum(points);
const groupSumX = (xs) => native.groupSumX(xs);
// fieldOp(op, a, b, {field, sharedB, montgomery, zeroOk}): batched field arithmetic on the device, the counterpart of the reference's
// bulkAddFields / bulkSubFields / bulkMulFields / bulkDoubleFields / bulkInvertFields / bulkPowFields / bulkPowFields17 / bulkSqrtFields.
// op: FIELD_OPS.add ..; a: n elements of 32 bytes (field 0: p, Aleo's `field`) or 48 (field 1: BLS12-377's q); b: n records, one with
// sharedB, or null for double / neg / square / inv / sqrt; an exponent is a 32-byte integer.  Resolves to the n results as a Buffer
// (canonical; the smaller square root).  Rejects for the inverse of 0 without zeroOk and for the root of a non-square: the Error has
// .index (the lowest failing element) and .reason (1 zero, 2 not a square).
const FIELD_OPS = { add: 0, sub: 1, mul: 2, double: 3, neg: 4, square: 5, inv: 6, pow: 7, sqrt: 8 };
const fieldOp = async (op, a, b, opts) => native.fieldOp(op, a, b === undefined ? null : b, opts);
// ntt(a, logN, {count, inverse, montgomery, shift}): `count` (default 1) number-theoretic transforms of 2^logN 32-byte elements of p each,
// natural order in and out -- arkworks' / snarkVM's radix-2 domains of BLS12-377's scalar field (te_msm_ntt).  shift: a 32-byte Buffer, the
// coset generator s; inverse undoes the forward with the same s; montgomery: a, s and the result are residues v * 2^256 mod p.  Resolves
// to the results as a Buffer (canonical); rejects for logN above 24 and for a shift that is 0 mod p.
const ntt = async (a, logN, opts) => native.ntt(a, logN, opts);

// polyDivide(a, n, z, {count, montgomery, sharedZ, quotient}): `count` (default 1) polynomials of n 32-byte coefficients of p each, lowest
// first, evaluated at their points z (one 32-byte record each, or one in all with sharedZ) and divided by X - z (te_msm_poly_divide):
// resolves to {evals, quotient} -- a(z) of each, and the coefficients of (a(X) - a(z)) / (X - z) at the stride n, the witness polynomial
// of a KZG opening (null with quotient: false).  montgomery: every record holds v * 2^256 mod p.  A refusal rejects.
const polyDivide = async (a, n, z, opts) => native.polyDivide(a, n, z, opts);

// fieldScan(op, a, n, {count, init, montgomery, exclusive, sharedA, out, totals}): the running sums (op 'sum') or products ('product') of
// `count` (default 1) vectors of n 32-byte records of p each -- one record each with sharedA: init * g^i, init + i g -- from their seeds
// init (one 32-byte record a vector; absent: 0 for the sum, 1 for the product) (te_msm_field_scan).  Resolves to {out, totals}: the running
// values at the stride n, a_i left out of value i with exclusive, and seed o a_0 o .. o a_(n-1) of each vector -- the closing value of a
// grand product; either is null when its option is false.  montgomery: every record holds v * 2^256 mod p.  A refusal rejects.
const SCAN_OPS = { sum: 0, product: 1 };
const fieldScan = async (op, a, n, opts) => {
  const code = typeof op === 'number' ? op : SCAN_OPS[op];
  if (code === undefined) throw new TypeError("fieldScan: op must be 'sum' or 'product'");
  return native.fieldScan(code, a, n, opts);
};

// bindMatrix(rows, cols, rowPtr, colIdx, vals, {montgomery, transpose}) binds a sparse matrix over p in CSR form -- rows + 1 offsets of 8
// bytes, nnz column indices of 4 bytes, nnz values of 32 bytes, little-endian Buffers -- and resolves to its id (te_msm_bind_matrix);
// spmv(id, x, {count, montgomery, transpose}) resolves to the products with `count` (default 1) vectors of cols 32-byte records each as a
// Buffer of count x rows canonical records (te_msm_spmv): the Az, Bz, Cz of an R1CS prover.  transpose multiplies by the transposed
// matrix (x: count x rows records) and needs a bind with transpose: true.  releaseMatrix(id) gives the matrix back.  A refusal rejects.
const bindMatrix = async (rows, cols, rowPtr, colIdx, vals, opts) => native.bindMatrix(rows, cols, rowPtr, colIdx, vals, opts);
const spmv = async (id, x, opts) => native.spmv(id, x, opts);
const releaseMatrix = (id) => native.releaseMatrix(id);

// Outside the reference's interface too: msmBatch(scalarBuffers) runs one MSM per Buffer over the set bound by setBases -- MSM m over
// its first scalarBuffers[m].length / 32 points (a prover's commitments to polynomials of different degrees against one SRS) -- and
// returns their results as [{x, y}, ...] in compute_msm's form, in input order.  Small MSMs share launch sequences on the GPU.
const msmBatch = (scalarBuffers) => {
  const out = native.msmBatch(scalarBuffers);
  const res = [];
  for (let m = 0; m < scalarBuffers.length; m++) res.push({ x: fromLE32(out, 64 * m), y: fromLE32(out, 64 * m + 32) });
  return res;
};

// And msmIndexed(indices, scalars): one MSM over an indexed subset of the set bound by setBases -- sum_j scalars[j] * P[indices[j]], a
// sparse witness or a strided range of the SRS without zero padding.  indices: a Uint32Array (any order, repeats allowed, each below the
// set's size); scalars: a Buffer of 32 bytes per index.  Resolves to {x, y} in compute_msm's form; rejects without setBases, on a scalar
// out of range, and on an index outside the set (the Error names the lowest offending position, also as .index).
const msmIndexed = async (indices, scalars) => {
  const out = native.msmIndexed(indices, scalars);
  return { x: fromLE32(out, 0), y: fromLE32(out, 32) };
};

module.exports = { compute_msm, setDevices, getDevices, setBases, getStats, setCheckPoints, setScalarsMontgomery, setScalarRecordBytes, setScalarBits, pointsFromX, scalarMul, scalarMulX, msmBatch, msmIndexed, setBase, scalarMulBase, groupAdd, groupAddX, groupSum, groupSumX, fieldOp, FIELD_OPS, ntt, polyDivide, bindMatrix, spmv, releaseMatrix, fieldScan, SCAN_OPS };
