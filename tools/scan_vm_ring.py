"""Check the built code of the kernels whose vector-memory requests are asm statements with hand-counted waits
(csrc/gru.hip: gru_bwd_direct_body, gru_fwd_direct_body) for the one thing the compiler cannot know: that no instruction reads
or writes a register between the load that targets it and the s_waitcnt vmcnt that covers it (a copy, a reuse as a temporary or
a second request would all go unnoticed by hipcc, which does not see the asm loads).

    hipcc --offload-arch=gfx950 [-DMMDFN_TUNING] -O3 -std=c++17 -I include -S mm_dfn_amd/csrc/gru.hip --cuda-device-only -o gru.s
    python tools/scan_vm_ring.py gru.s gru_seq_fwd_io_kernelILi0ELi0ELi0ELi1E gru_seq_fwd_io_flags_kernelILi1E

Every path of a kernel's control flow is walked (loops at most twice; s_cbranch_execz is taken as never taken: the stores of
these bodies are issued by every wave, which is what their wait counts rely on).  Along a path the queue of vector-memory
operations is kept; vector-memory operations retire in order, so an s_waitcnt vmcnt(N) retires all but the last N; any
instruction that touches the destination of a load still in the queue is reported.  Prints the vmcnt immediates met on the
shortest and the longest paths.  Exit status 1 if anything was reported."""
import re
import sys

sys.setrecursionlimit(100000)
MAX_BRANCHES = 20000       # (the direct recurrence bodies need a few hundred)


def regs(text):
    out = set()
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", text):
        if m.group(1):
            out.update(range(int(m.group(1)), int(m.group(2)) + 1))
        else:
            out.add(int(m.group(3)))
    return out


def kernel_text(lines, key):
    starts = [i for i, l in enumerate(lines) if re.match(r"[A-Za-z_]\w*:", l) and key in l.split(":")[0]]
    if not starts:
        raise SystemExit("no kernel matching %r" % key)
    i = starts[0]
    j = next(k for k in range(i, len(lines)) if lines[k].startswith(".Lfunc_end"))
    return lines[i].split(":")[0], [l.split(";")[0].strip() for l in lines[i + 1:j]]


def scan(name, code):
    label = {}
    for i, t in enumerate(code):
        m = re.match(r"(\.LBB\d+_\d+):", t)
        if m:
            label[m.group(1)] = i
    hazards, sequences, paths, calls = set(), set(), [0], [0]

    def walk(pc, queue, visits, imm):
        calls[0] += 1
        if calls[0] > MAX_BRANCHES:
            raise SystemExit("%s: more than %d branches walked (a kernel with nested data-dependent control flow): not scanned"
                             % (name, MAX_BRANCHES))
        queue, imm = list(queue), list(imm)
        while pc < len(code):
            t = code[pc]
            m = re.match(r"(\.LBB\d+_\d+):", t)
            if m:
                visits = dict(visits)
                visits[m.group(1)] = visits.get(m.group(1), 0) + 1
                if visits[m.group(1)] > 2:
                    return
            elif not t or t.startswith("."):
                pass
            elif t.startswith("s_endpgm"):
                paths[0] += 1
                sequences.add(tuple(imm))
                return
            elif t.startswith("s_cbranch_"):
                kind, target = re.match(r"s_cbranch_(\w+)\s+(\S+)", t).groups()
                if kind != "execz":
                    walk(label[target], queue, visits, imm)
            elif t.startswith("s_branch"):
                pc = label[t.split()[1]]
                continue
            elif t.startswith("s_waitcnt"):
                m = re.search(r"vmcnt\((\d+)\)", t)
                if m:
                    n = int(m.group(1))
                    imm.append(n)
                    queue = queue[max(0, len(queue) - n):] if n else []
            else:
                in_flight = set().union(*queue) if queue else set()
                if regs(t) & in_flight:
                    hazards.add((pc + 1, t))
                m = re.match(r"global_load_\w+\s+(\S+),", t)
                if m:
                    queue.append(regs(m.group(1)))
                elif re.match(r"(global|buffer|scratch|flat)_(store|atomic)", t):
                    queue.append(set())
            pc += 1

    walk(0, [], {}, [])
    print("%s: %d paths, %d hazards" % (name, paths[0], len(hazards)))
    for line, text in sorted(hazards)[:40]:
        print("    line %d of the kernel: %s" % (line, text))
    by_len = sorted(sequences, key=len)
    for s in by_len[:2] + by_len[-1:]:
        print("    vmcnt immediates of a path:", list(s))
    return len(hazards)


if __name__ == "__main__":
    if len(sys.argv) < 3:
        raise SystemExit(__doc__)
    lines = open(sys.argv[1]).read().split("\n")
    bad = 0
    for key in sys.argv[2:]:
        bad += scan(*kernel_text(lines, key))
    sys.exit(1 if bad else 0)
