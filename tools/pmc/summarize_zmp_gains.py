"""Per wave-tick PMC of the tick kernels with and without ZMP gain scheduling (profiles/r06_tick_zmp_gains_pmc.json).

    # on the GPU machine, one run per counter set (kernel trace only):
    rocprofv3 --pmc <set> --kernel-trace --output-format csv -d DIR/pmcN -o pmc -- \
        python tools/tick_controller_timing.py --zmp-gain-scheduling --no-check --reps 1 --ticks 200
    python tools/pmc/summarize_zmp_gains.py DIR OUT.json
"""
import csv, glob, collections, json, sys
tot=collections.defaultdict(lambda: collections.defaultdict(float)); disp=collections.defaultdict(set)
for f in glob.glob(sys.argv[1] + '/pmc*/*counter_collection.csv'):
    for r in csv.DictReader(open(f)):
        k=r['Kernel_Name'].replace('void (anonymous namespace)::','').split('(')[0]
        if not ('ik4_tick_gs_kernel' in k or 'ik4_kernel<true' in k or 'ik4_tick_reactive_kernel' in k): continue
        tot[k][r['Counter_Name']]+=float(r['Counter_Value'])
        disp[k].add((f.split('/')[-2], r['Dispatch_Id']))
TICKS, B = 216, 8192
WT = TICKS * B / 4          # wave-ticks (4 robots per wave)
pairs=[("constant_jacobians","mpc","ik4_kernel<true, 0, false, false>","ik4_tick_gs_kernel<0, false, false, false>"),
       ("constant_jacobians","reactive","ik4_tick_reactive_kernel<0, false, false>","ik4_tick_gs_kernel<0, false, false, true>"),
       ("fused_kinematics","mpc","ik4_kernel<true, 2, false, false>","ik4_tick_gs_kernel<2, false, false, false>"),
       ("fused_kinematics","reactive","ik4_tick_reactive_kernel<2, false, false>","ik4_tick_gs_kernel<2, false, false, true>")]
per_wave=["SQ_INSTS_VALU","SQ_INSTS_SALU","SQ_INSTS_SMEM","SQ_INSTS_VMEM_RD","SQ_INSTS_VMEM_WR","SQ_INSTS_LDS","SQ_WAVE_CYCLES","SQ_WAIT_INST_ANY","SQ_WAIT_ANY","SQ_ACTIVE_INST_ANY"]
out={"what": "PMC of the tick kernels with and without ZMP gain scheduling: tools/tick_controller_timing.py --zmp-gain-scheduling --no-check --reps 1 --ticks 200 under rocprofv3 --pmc <set> --kernel-trace, one run per counter set; 8192 robots, 216 ticks per kernel (16 warm-up + 200). SQ_* per wave-tick (4 robots per wave), FETCH_SIZE / WRITE_SIZE in bytes per robot-tick, GRBM_GUI_ACTIVE in GPU cycles per tick",
     "pairs": []}
for form,ctrl,twin,gs in pairs:
    row={"form":form,"dcm_controller":ctrl,"twin":twin,"scheduled":gs,"counters":{}}
    for c in per_wave+["FETCH_SIZE","WRITE_SIZE","GRBM_GUI_ACTIVE"]:
        a,b=tot[twin][c],tot[gs][c]
        if c in per_wave: a,b=a/WT,b/WT
        elif c=="GRBM_GUI_ACTIVE": a,b=a/TICKS,b/TICKS
        else: a,b=a*1024/(TICKS*B),b*1024/(TICKS*B)
        row["counters"][c]={"twin":round(a,2),"scheduled":round(b,2),"ratio":round(b/a,4) if a else None}
    out["pairs"].append(row)
json.dump(out,open(sys.argv[2],'w'),indent=1)
for r in out["pairs"]:
    print(r["form"],r["dcm_controller"])
    for c,v in r["counters"].items(): print("   %-20s %12s %12s %s"%(c,v["twin"],v["scheduled"],v["ratio"]))
