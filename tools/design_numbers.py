"""Regenerate the end-of-round numbers block of DESIGN.md section 7 (between the `numbers:begin` / `numbers:end` markers) from the committed
bench lines (profiles/r6_*.json), so that the text quotes exactly what the files hold (tests/test_docs.py checks it):
    python tools/design_numbers.py"""
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = lambda n: json.load(open(os.path.join(ROOT, "profiles", n)))  # noqa: E731
BEGIN, END = "<!-- numbers:begin -->", "<!-- numbers:end -->"


def block():
    line, cfg4 = P("r6_bench_line.json"), P("r6_bench_cfg4_line.json")
    rf, it = line["roofline"], line["roofline"]["per_gru_iteration"]
    cp, sw, cb, cv = rf["ceiling_probe"], line["batch_sweep_ms_per_map"], line["cpu_baseline"], line["roofline_conv2d"]
    tr = rf["traffic"]
    rg = cp["random_line_gather"]
    return f"""End-of-round numbers (1 x MI355X, `profiles/r6_bench_line.json` = the full line (`python bench.py --full --conv-table`) of the round's last GPU session,
`tools/sessions/r6_final.sh`: the whole GPU suite with `-x` green, `smoke()`, this command, the rocprofv3 kernel stats and PMC passes of the same
command, the second lines; no `csrc/` / `include/` change after it): **{round(line['value'])} depth-maps/s** at the default 96 reference views per step
({line['ms_per_step']:.1f} ms per step, `conv_arith` = {line['config'].get('conv_arith')}; round 5: 1313 / 73.1 on the driver's run, round 4: 1299, round 3: 1200, round 2: 1118, round 1: 848 at B=16;
box-to-box spread of one build ~2 %: 1472 / 1494 / 1501 in other sessions of the same kernels).
`roofline.frac` {rf['frac']:.2f} ({rf['avg_launch_us']:.0f} us per launch; first GRU iteration {it[0]['frac']:.2f}, iterations 2-4 {min(x['frac'] for x in it[1:]):.3f}-{max(x['frac'] for x in it[1:]):.3f};
`traffic` {('%.2f GB' % (tr / 1e9)) if tr else 'n/a'} per launch against {rf['algorithmic_bytes_per_launch'] / 1e9:.2f} GB algorithmic; `ceiling_probe_us` {rf['ceiling_probe_us']:.0f} in-step,
measured by this process: product / probe {cp['product_over_probe_in_step']:.2f} in-step, {cp['product_over_probe_isolated']:.2f} isolated; the 0.60 mark is {cp['gate_0p60_us']:.0f} us;
random 128-byte lines: {rg['every_line_once']['requested_GBs'] / 1e3:.1f} TB/s once each, {rg['band48_8_per_quad']['us']:.0f} us for the band pattern),
`roofline_scene_geometry.frac` {line['roofline_scene_geometry']['frac']:.2f}, `roofline_warp_init.frac` {line['roofline_warp_init']['frac']:.2f},
`roofline_conv2d.frac` {cv['frac']:.2f} over {100 * cv['share_of_step_time']:.0f} % of the step ({cv['ms_by_binding_roof']['mfma']:.1f} ms in matrix-bound rows, {cv['ms_by_binding_roof']['hbm']:.1f} ms in HBM-bound rows,
{cv['hbm_achieved_GBs'] / 1e3:.2f} TB/s of algorithmic traffic over the family).
By batch {sw['16']['eager_ms_per_map']:.2f} ms per map at B=16, {sw['32']['eager_ms_per_map']:.2f} at 32, {sw['64']['eager_ms_per_map']:.2f} at 64; batch 1 {sw['1']['eager_ms_per_map']:.2f} eager / {sw['1']['graph_ms_per_map']:.2f} graphed.
CPU baseline {cb['value']:.2f} maps/s (oracle port, {cb['cores']} threads) => ~{round(line['value'] / cb['value'] / 10) * 10}x -- a reported baseline, not a kernel-quality figure.
Training step (`profiles/r6_bench_cfg4_line.json`): **{cfg4['value']:.1f} samples/s** ({cfg4['ms_per_step']:.1f} ms per step; `getcost_bwd` {cfg4['roofline_getcost_bwd']['ms_per_step']:.1f} ms,
`conv2d_wgrad` {cfg4['roofline_conv2d_wgrad']['ms_per_step']:.1f} ms at {cfg4['roofline_conv2d_wgrad']['frac']:.2f} of the fp32-MFMA peak); round 5: 31.4.
The previous review's gates, as measured: step <= 69 ms: **{'met' if line['ms_per_step'] <= 69.0 else 'not met'}** ({line['ms_per_step']:.1f}); conv2d >= 0.68 of the fp32-MFMA peak:
**{'met' if cv['frac'] >= 0.68 else 'not met'}** ({cv['frac']:.2f}, with the split-bf16 arithmetic of 4.5 priced against the fp32 peak); GetCost probe numbers on the driver's line: met;
batch 1 <= 2.4 ms graphed: {'met' if sw['1']['graph_ms_per_map'] <= 2.4 else 'not met'} ({sw['1']['graph_ms_per_map']:.2f}); cfg4 >= 36 samples/s: **met** ({cfg4['value']:.1f}); plane sweep >= 0.34: not met
({line['roofline_warp_init']['frac']:.2f}; the 8-wave form measured slower and closed, section 11)."""


def main():
    p = os.path.join(ROOT, "DESIGN.md")
    s = open(p).read()
    a, b = s.index(BEGIN) + len(BEGIN), s.index(END)
    s = s[:a] + "\n" + block() + "\n" + s[b:]
    open(p, "w").write(s)
    print("DESIGN.md numbers block regenerated")


if __name__ == "__main__":
    main()
