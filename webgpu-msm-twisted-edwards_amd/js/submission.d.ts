// Type declaration matching the reference's export (submission/submission.ts:73-78).
export interface BigIntPoint { x: bigint; y: bigint; t: bigint; z: bigint; }
export interface U32ArrayPoint { x: Uint32Array; y: Uint32Array; t: Uint32Array; z: Uint32Array; }
export declare const compute_msm: (
  bufferPoints: BigIntPoint[] | U32ArrayPoint[] | Buffer,
  bufferScalars: bigint[] | Uint32Array[] | Buffer,
  log_result?: boolean,
  force_recompile?: boolean,
) => Promise<{ x: bigint; y: bigint }>;
// Not in the reference: the GPUs a call is sharded over (default: TE_MSM_DEVICES, else device 0).
export declare const setDevices: (ids: number[]) => void;
export declare const getDevices: () => number[];
// Not in the reference: resident bases.  setBases(points) binds that Buffer once (upload + conversion on every device);
// compute_msm(points, scalars) with the same Buffer object then moves the scalars only (full_benchmarks.ts:63-68,100-105 pass
// one point buffer to six calls per size).  setBases(null) unbinds.
// { montgomery: true }: the coordinates are Montgomery residues x * 2^256 mod p (a native prover's in-memory form); same set, same results.
// { stride: s }: point i starts at byte i * s (a multiple of 8 in [64, 128]; bytes behind x || y are not interpreted).  { infinityFlag: true } is
// the engine's BLS12-377 option "point_infinity_flag": on this addon's curve setBases throws (te_msm error -1).  All are remembered per buffer.
export declare const setBases: (bufferPoints: Buffer | null, options?: { montgomery?: boolean, stride?: number, infinityFlag?: boolean }) => void;
// Not in the reference: the scalar buffers of later compute_msm / msmBatch / msmIndexed calls hold Montgomery residues k * 2^256 mod L,
// decoded on the GPU (any 256-bit value stands for its residue); scalarMul / scalarMulX throw while it is set.
export declare const setScalarsMontgomery: (flag: boolean) => void;
// Not in the reference: the engine's option "scalar_record_bytes" for later calls: 0 = the curve's own scalar record (32 bytes here), 32 the
// same spelled out; 48 is BLS12-377's record, under which every call of this addon that reads scalars rejects (te_msm error -1).
export declare const setScalarRecordBytes: (n: 0 | 8 | 16 | 32 | 48) => void;
// Not in the reference: the engine's option "scalar_bits" for later calls: every scalar is below 2^b (0 = nothing declared).  With 8 / 16 above
// the scalar buffers of compute_msm, msmBatch and msmIndexed are native u64 / u128 arrays; 8 stands for b = 64, 16 needs setScalarBits(1..128).
export declare const setScalarBits: (b: number) => void;
export declare const getStats: () => { submittedInEnter: number; submittedInExecute: number; loneRuns: number; boundJobs: number; maxInFlight: number };
// Not in the reference: opt-in validation of input points (0 none, 1 canonical + on the curve, 2 + prime-order subgroup); a bad
// point rejects the call's promise (the message names the index and the reason), setBases throws for a bad set.
export declare const setCheckPoints: (level: 0 | 1 | 2) => void;
// Not in the reference: x-only points (Aleo group values, Address.msm's input) -> the 64n-byte points buffer of compute_msm /
// setBases, y recovered on the GPU; a bad x throws (the message names the index and the reason; also error.index / error.reason).
export declare const pointsFromX: (xs: Buffer) => Buffer;
// Not in the reference: batch scalar multiplication, [k_i] P_i for every i (no sum) as a 64n-byte points Buffer; scalarMulX takes
// x-only points (bulkGroupScalarMul).  One 32-byte scalar is shared by all points; a bad point or x throws (error.index / error.reason).
export declare const scalarMul: (points: Buffer, scalars: Buffer) => Buffer;
export declare const scalarMulX: (xs: Buffer, scalars: Buffer) => Buffer;
// Not in the reference: fixed-base batch scalar multiplication.  setBase binds one 64-byte point (a table built once); scalarMulBase
// returns [k_i] P for n 32-byte scalars as a 64n-byte points Buffer.  setScalarsMontgomery applies to these scalars.
export declare const setBase: (point: Buffer) => void;
export declare const scalarMulBase: (scalars: Buffer) => Buffer;
// Not in the reference's interface: batched group addition and point-set sums on the device (its bulkAddGroups / reduceGroups run on the
// CPU).  groupAdd returns the 64n-byte points A_i + B_i (A_i - B_i with subtract); one 64-byte b is shared by every a.  groupAddX /
// groupSumX take x-only points.  groupSum returns 64 bytes x || y.  A bad point or x throws (error.index / error.reason / error.operand).
export declare const groupAdd: (a: Buffer, b: Buffer, opts?: { subtract?: boolean }) => Buffer;
export declare const groupAddX: (ax: Buffer, bx: Buffer, opts?: { subtract?: boolean }) => Buffer;
export declare const groupSum: (points: Buffer) => Buffer;
export declare const groupSumX: (xs: Buffer) => Buffer;
// Not in the reference's interface: batched field arithmetic on the device (its bulk*Fields run on the CPU, one WASM call per element).
// a: n elements of 32 bytes (field 0: p, Aleo's `field`) or 48 (field 1: BLS12-377's base field); b: n records, ONE with sharedB, or null
// for double / neg / square / inv / sqrt; an exponent is a 32-byte integer (bulkPowFields17: pow, sharedB, b = 17).  montgomery: inputs
// and outputs are residues v * 2^256 mod p / v * 2^384 mod q.  Resolves to the n canonical results (sqrt: the smaller root).  The inverse
// of 0 without zeroOk and the root of a non-square reject with an Error whose .index is the lowest failing element and .reason 1 / 2.
export declare const FIELD_OPS: { add: 0, sub: 1, mul: 2, double: 3, neg: 4, square: 5, inv: 6, pow: 7, sqrt: 8 };
export declare const fieldOp: (op: number, a: Buffer, b?: Buffer | null,
  opts?: { field?: 0 | 1, sharedB?: boolean, montgomery?: boolean, zeroOk?: boolean }) => Promise<Buffer>;
// Not in the reference: batched NTTs over p on the device -- `count` (default 1) transforms of 2^logN 32-byte elements each, natural order
// in and out, the radix-2 domains of arkworks / snarkVM over BLS12-377's scalar field.  shift: one 32-byte record, the coset generator;
// inverse undoes the forward with the same shift; montgomery as for fieldOp.  Rejects for logN above 24 and a shift that is 0 mod p.
export declare const ntt: (a: Buffer, logN: number,
  opts?: { count?: number, inverse?: boolean, montgomery?: boolean, shift?: Buffer }) => Promise<Buffer>;
// Not in the reference: polynomial openings over p on the device -- `count` (default 1) polynomials of n 32-byte coefficients each, lowest
// first, evaluated at their points z (one 32-byte record each, or one in all with sharedZ) and divided by X - z.  evals: a(z) of each;
// quotient: the coefficients of (a(X) - a(z)) / (X - z) at the stride n (the last one 0), the witness polynomial of a KZG opening, or null
// with quotient: false.  montgomery as for fieldOp.  Rejects for n = 0 and n above 2^30.
export declare const polyDivide: (a: Buffer, n: number, z: Buffer,
  opts?: { count?: number, montgomery?: boolean, sharedZ?: boolean, quotient?: boolean }) => Promise<{ evals: Buffer, quotient: Buffer | null }>;
// Not in the reference: prefix sums ('sum') and products ('product') over p on the device -- `count` (default 1) vectors of n 32-byte
// records each (one record each with sharedA) from their seeds init (one record a vector; absent: the identity).  out: the running values at
// the stride n (exclusive leaves a_i out of value i); totals: seed o a_0 o .. o a_(n-1) of each vector; either is null when its option is
// false.  montgomery as for fieldOp.  Rejects for an unknown op, n = 0 and n above 2^30.
export declare const SCAN_OPS: { sum: 0, product: 1 };
export declare const fieldScan: (op: 'sum' | 'product' | number, a: Buffer, n: number,
  opts?: { count?: number, init?: Buffer, montgomery?: boolean, exclusive?: boolean, sharedA?: boolean, out?: boolean, totals?: boolean }) => Promise<{ out: Buffer | null, totals: Buffer | null }>;
// Not in the reference: sparse matrices over p bound once in CSR form (rowPtr: rows + 1 offsets of 8 bytes, colIdx: nnz indices of 4 bytes,
// vals: nnz records of 32 bytes, little-endian), and their products with `count` (default 1) vectors of cols records each: count x rows
// canonical records.  transpose multiplies by the transposed matrix and needs a bind with transpose: true; montgomery as for fieldOp (on the
// bind: the values; on spmv: x and the result).  Rejects for rows or cols 0, a column index >= cols, and a released id.
export declare const bindMatrix: (rows: number, cols: number, rowPtr: Buffer, colIdx: Buffer, vals: Buffer,
  opts?: { montgomery?: boolean, transpose?: boolean }) => Promise<number>;
export declare const spmv: (id: number, x: Buffer, opts?: { count?: number, montgomery?: boolean, transpose?: boolean }) => Promise<Buffer>;
export declare const releaseMatrix: (id: number) => void;
// Not in the reference: batched MSMs over prefixes of the set bound by setBases; MSM m runs over the first scalarBuffers[m].length / 32
// points.  Results in input order, in compute_msm's form; throws without setBases or for a buffer longer than the set.
export declare const msmBatch: (scalarBuffers: Buffer[]) => { x: bigint; y: bigint }[];
// Not in the reference: one MSM over an indexed subset of the set bound by setBases, sum_j scalars[j] * P[indices[j]] (indices in any
// order, repeats allowed, each below the set's size; 32 scalar bytes per index).  Rejects without setBases, for a scalar out of range and
// for an index outside the set (the Error's .index is the lowest offending position).
export declare const msmIndexed: (indices: Uint32Array, scalars: Buffer) => Promise<{ x: bigint; y: bigint }>;
