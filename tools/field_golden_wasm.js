// Runs the reference's own field arithmetic -- Address.add_fields / sub_fields / mul_fields / double_field / invert_field / pow_field /
// sqrt of the prebuilt Aleo WASM, the bodies of bulk*Fields (reference utils/wasmFunctions.ts) -- under node, where the reference tree
// is present.  Nothing of the reference is copied: the glue and the .wasm are read from TE_REFERENCE_ROOT at run time.
// usage: node field_golden_wasm.js <cases.json> <out.json>     (tools/gen_field_golden.py writes the cases and files the answers)
//   cases.json: [{op, a: decimal, b: decimal or absent}, ...]  ->  out.json: the same with out: decimal, or "traps"
const fs = require("fs");
if (!process.env.TE_REFERENCE_ROOT) { console.error("TE_REFERENCE_ROOT must name the reference tree"); process.exit(2); }
const dir = process.env.TE_REFERENCE_ROOT + "/src/reference/wasm-loader/";
const names = [];
let src = fs.readFileSync(dir + "aleo_wasm_bg.js", "utf8")
  .replace(/^export function (\w+)/gm, (m, n) => (names.push(n), "function " + n))
  .replace(/^export class (\w+)/gm, (m, n) => (names.push(n), "class " + n));
src += "\nmodule.exports={" + names.join(",") + "};";
const wasm = new WebAssembly.Module(fs.readFileSync(dir + "aleo_wasm_bg.wasm"));
// a trap leaves the instance, and the glue's views of its memory, in an unknown state: the next case gets both afresh
function fresh() {
  const mod = { exports: {}, require };
  new Function("module", "exports", "require", src)(mod, mod.exports, require);
  const glue = mod.exports;
  const inst = new WebAssembly.Instance(wasm, { "./aleo_wasm_bg.js": glue });
  glue.__wbg_set_wasm(inst.exports);
  return glue.Address;
}
const f = (v) => v + "field";
const call = {
  add: (A, c) => A.add_fields(f(c.a), f(c.b)),
  sub: (A, c) => A.sub_fields(f(c.a), f(c.b)),
  mul: (A, c) => A.mul_fields(f(c.a), f(c.b)),
  double: (A, c) => A.double_field(f(c.a)),
  inv: (A, c) => A.invert_field(f(c.a)),
  pow: (A, c) => A.pow_field(f(c.a), f(c.b)),
  sqrt: (A, c) => A.sqrt(f(c.a)),
};
const cases = JSON.parse(fs.readFileSync(process.argv[2], "utf8"));
let A = fresh();
for (const c of cases) {
  try {
    c.out = call[c.op](A, c).replace("field", "");
  } catch (e) {
    c.out = "traps";
    A = fresh();
  }
}
fs.writeFileSync(process.argv[3], JSON.stringify(cases));
