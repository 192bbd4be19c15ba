"""The child process of tests/test_gpu_threads.py:  python tests/thread_driver.py WORKDIR

Reads WORKDIR/scenes.pkl (tests/thread_scenes.py build(), written by the parent: the proofs are made once, there), plays the scenes one
after another in this one process and writes WORKDIR/<scene>.json: every call's result (or its error code and text) with its entry and
exit time, the alone-replay of the first mismatching calls, and per C symbol how many threads were inside it at once.  The symbols are
counted by proxies around the attributes of _lib.load_library(), put in place once before the first context is made.

Before each call a thread writes what it is about to do into its progress slot.  The main thread waits for a scene's threads with a
deadline; on expiry it writes the slots to WORKDIR/stuck.json and leaves with os._exit(3), and a thread that meets H2V_ERR_DEVICE
anywhere ends the driver the same way with os._exit(4).  No further scene is started, and nothing here repeats a call until
something goes wrong: threads are daemons and every loop runs over a list made before the start."""
import ctypes
import json
import os
import pickle
import sys
import threading
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import thread_scenes as ts   # noqa: E402

DEADLINE_S = 30.0
REPLAYS = 3          # mismatching calls replayed alone, per scene


class CountingLib:
    """the C library with every symbol of _lib.SIGNATURES behind a proxy that counts the threads inside it"""

    def __init__(self, lib, names):
        self._mu = threading.Lock()
        self.inside, self.peak, self.calls, self.scene = {}, {}, {}, None
        for name in names:
            setattr(self, name, self._proxy(name, getattr(lib, name)))

    def _proxy(self, name, fn):
        mu, inside = self._mu, self.inside
        inside[name] = 0

        def proxy(*args):
            with mu:
                inside[name] += 1
                key = (self.scene, name)
                self.calls[key] = self.calls.get(key, 0) + 1
                if inside[name] > self.peak.get(key, 0):
                    self.peak[key] = inside[name]
            try:
                return fn(*args)
            finally:
                with mu:
                    inside[name] -= 1
        return proxy

    def report(self, scene):
        return {name: {"calls": n, "peak": self.peak[(s, name)]} for (s, name), n in sorted(self.calls.items(), key=str) if s == scene}


class Player:
    def __init__(self, workdir, data):
        import halo2_verifier_amd as h2v
        from halo2_verifier_amd import _lib
        self.h2v, self.workdir, self.keys, self.check = h2v, workdir, data["keys"], _lib.check
        self.lib = CountingLib(_lib.load_library(), list(_lib.SIGNATURES))
        _lib._LIB = self.lib          # every Context made from here on calls through the proxies
        self.progress = {}
        self.device_error = threading.Event()

    # ------------------------------------------------------------------ objects
    def make(self, rep):
        h2v = self.h2v
        env = {}
        for name, key in rep["contexts"]:
            params, vk = self.keys[key]
            env[name] = h2v.Context(h2v.ParamsKZG(params, h2v.SerdeFormat.RawBytes), h2v.VerifyingKey(vk, h2v.SerdeFormat.RawBytes))
        for spec in rep["objects"]:
            env[spec[0]] = self.make_object(env, spec)
        return env

    def make_object(self, env, spec):
        h2v = self.h2v
        name, kind, ctx, init = spec
        if kind == "batch":
            return h2v.Batch(env[ctx], init["max_proofs"], init["values"], groups=init["groups"])
        if kind == "acc":
            return h2v.Accumulator(env[ctx])
        if kind == "msm":
            m = h2v.MSMKZG(env[ctx])
            if init.get("terms"):
                m.append_terms(*init["terms"])
            return m
        if kind == "dual":
            d = h2v.DualMSM(env[ctx])
            d.add_msm(init["guard"])
            return d
        raise ValueError(kind)

    def close(self, rep, env):
        for spec in reversed(rep["objects"]):
            env[spec[0]].close()
        for name, _ in rep["contexts"]:
            env[name].close()

    # ------------------------------------------------------------------ arguments that live on the device, made before the start
    def prepare(self, c):
        import torch
        a = c["args"]
        if c["op"] == "b_upload_tensors":
            n = a["n"]
            dev = lambda data, width: torch.frombuffer(bytearray(data), dtype=torch.uint8).reshape(n, width).cuda()
            return (dev(a["proofs"], a["proof_len"]), dev(a["instances"], 32 * sum(a["col_lens"])), dev(a["rand"], 32))
        if c["op"] == "b_finish_into":
            n, g = a["n"], a["groups"]
            full = lambda count, dtype: torch.full((count,), 0xEE if dtype == torch.uint8 else -286331154, dtype=dtype, device="cuda:0")
            return {"status": full(n, torch.int32), "group_ok": full(g, torch.int32), "left_xy": full(64 * g, torch.uint8).reshape(g, 64),
                    "right_xy": full(64 * g, torch.uint8).reshape(g, 64), "group_failed": full(g, torch.int32), "summary": full(8, torch.int32)}
        if c["op"] == "b_export":
            return torch.zeros(a["groups"] * ts.ACC_RECORD_BYTES, dtype=torch.uint8, device="cuda:0")
        if c["op"] == "b_set_stream":
            return torch.cuda.Stream()
        return None

    # ------------------------------------------------------------------ one call
    def run(self, env, c, prepared=None):
        h2v = self.h2v
        op, a = c["op"], c["args"]
        on = c["on"]
        obj = [env[x] for x in on] if isinstance(on, list) else env[on]
        if op in ("verify_batch", "verify_batch_shapes"):
            return obj.verify_batch(a["proofs"], a["instances"], a["rand"])
        if op == "verify_batch_seeded":
            return obj.verify_batch(a["proofs"], a["instances"], a["rand"], seed=a["seed"])
        if op == "verify_batch_identify":
            return obj.verify_batch_identify(a["proofs"], a["instances"], a["rand"])
        if op == "verify_batches":
            return obj.verify_batches(a["batches"], a["rand"])
        if op == "verify_each":
            return obj.verify_each(a["proofs"], a["instances"])
        if op == "verify_batch_keys":
            return h2v.verify_batch_keys(obj, a["keys"], a["proofs"], a["instances"], a["rand"])
        if op == "guard_msm":
            return obj.guard_msm(a["proof"], a["instances"])
        if op == "guards_check_each":
            return obj.guards_check_each(a["guards"])
        if op == "msm_g1":
            return obj.msm_g1(a["scalars"], a["bases"])
        if op == "pairing_check":
            return obj.pairing_check(a["left"], a["right"])
        if op == "msm_append":
            return obj.append_terms(a["scalars"], a["bases"])
        if op == "msm_scale":
            return obj.scale(a["factor"])
        if op == "msm_scalars":
            return obj.scalars()
        if op == "msm_add_msm":
            return obj[0].add_msm(obj[1])
        if op == "msm_eval_many":
            return h2v.eval_many(obj)
        if op == "dual_check_many":
            return h2v.dual_check_many(obj)
        if op == "b_set_groups":
            for _ in range(a.get("repeat", 1)):
                obj.set_groups(a["groups"])
            return None
        if op == "b_set_group_sizes":
            return obj.set_group_sizes(a["sizes"])
        if op == "b_upload":
            return obj.upload(a["proofs"], a["proof_len"], a["instances"], a["col_lens"], a["rand"])
        if op == "b_upload_launch":
            return obj.upload_launch(a["proofs"], a["proof_len"], a["instances"], a["col_lens"], a["rand"], with_pairing=a["pairing"])
        if op == "b_upload_tensors":
            proofs, insts, tail = prepared if prepared is not None else self.prepare(c)
            return obj.upload_tensors(proofs, insts, a["col_lens"], tail)
        if op == "b_launch":
            return obj.launch(with_pairing=a["pairing"])
        if op == "b_finish":
            return obj.finish()
        if op == "b_finish_groups":
            return obj.finish_groups()
        if op == "b_finish_into":
            import torch
            t = prepared if prepared is not None else self.prepare(c)
            obj.finish_into(**t)
            torch.cuda.current_stream().synchronize()      # (finish_into made this stream wait for the batch's)
            g = a["groups"]
            points = lambda k: [bytes(t[k][i].cpu().numpy().tobytes()) for i in range(g)]
            return {"status": t["status"].tolist(), "group_ok": t["group_ok"].tolist(), "left_xy": points("left_xy"), "right_xy": points("right_xy"),
                    "group_failed": [v & 0xffffffff for v in t["group_failed"].tolist()], "summary": [v & 0xffffffff for v in t["summary"].tolist()]}
        if op == "b_recheck":
            return obj.recheck(a["ranges"])
        if op == "b_identify":
            return obj.identify()[:2]
        if op == "a_process":
            ctxs = [env[x] for x in a["contexts"]] if isinstance(a["contexts"], list) else env[a["contexts"]]
            return obj.process(ctxs, a["keys"], a["proofs"], a["instances"], a["rand"])
        if op == "a_process_guards":
            return obj.process_guards(a["guards"], a["rand"])
        if op == "a_process_batch":
            return obj.process_batch(env[a["batch"]])
        if op == "a_add_msm":
            return obj.add_msm(a["left"], a["right"])
        if op == "a_read":
            return obj.read()
        if op == "a_finalize":
            return obj.finalize()
        if op == "a_merge":
            return obj.merge([env[x] for x in a["sources"]], a["draws"])
        if op == "a_export_state":
            return obj.export_state()
        if op == "verify_batch_seeded_identify":
            return obj.verify_batch_identify(a["proofs"], a["instances"], a["rand"], seed=a["seed"])
        if op == "verify_batch_keys_identify":
            return h2v.verify_batch_keys_identify(obj, a["keys"], a["proofs"], a["instances"], a["rand"])[:4]
        if op == "a_add_msms":
            return obj.add_msms(env[a["dual"]])
        if op == "b_recheck_many":
            return h2v.recheck_batches([obj], a["ranges"])
        if op == "b_accumulators":
            ptr, nbytes = ctypes.c_void_p(), ctypes.c_size_t(0)
            self.check(self.lib.h2v_batch_accumulators(obj._h, ctypes.byref(ptr), ctypes.byref(nbytes)))
            return nbytes.value
        if op == "b_export":
            import torch
            env[a["rec"]] = prepared if prepared is not None else self.prepare(c)
            obj.export_accumulators(env[a["rec"]].data_ptr())
            torch.cuda.synchronize()                       # (the record is read on other streams)
            return None
        if op == "fold_check":
            ok, left, right = ctypes.c_int(0), ctypes.create_string_buffer(64), ctypes.create_string_buffer(64)
            self.check(self.lib.h2v_fold_check(obj._h, ctypes.c_void_p(env[a["rec"]].data_ptr()), 1, ctypes.byref(ok), left, right))
            return bool(ok.value), left.raw, right.raw
        if op == "b_fold_enqueue":
            return obj.fold_check_enqueue(env[a["rec"]].data_ptr(), 1)
        if op == "b_set_stream":
            env[a["stream"]] = prepared if prepared is not None else self.prepare(c)
            return obj.set_stream(env[a["stream"]].cuda_stream)
        if op == "b_stream":
            return all([bool(obj.stream) for _ in range(a["repeat"])])
        if op == "a_journal_begin":
            return obj.journal_begin(a["capacity"])
        if op == "a_check_legs":
            return obj.check_legs()
        if op == "a_drop_legs":
            return obj.drop_legs(a["legs"])
        if op == "a_merge_states":
            return obj.merge_states(a["states"], a["draws"])
        if op == "merge_local":
            from halo2_verifier_amd import distributed
            return distributed.merge_accumulators_local(obj, [env[x] for x in a["sources"]], a["draws"])
        raise ValueError(op)

    def record(self, env, c, prepared=None):
        """-> the call's record: times, the result or the error, and whether that is what the scene expects"""
        t0 = time.perf_counter_ns()
        try:
            got, err = ts.canon(self.run(env, c, prepared)), None
        except self.h2v.H2VError as e:
            got, err = None, [e.code, str(e)]
        t1 = time.perf_counter_ns()
        if err is not None and err[0] == ts.ERR_DEVICE:
            self.device_error.set()
        if c["error"] is not None:
            ok = err is not None and err[0] == c["error"][0] and err[1].endswith(c["error"][1])
        else:
            ok = err is None and ts.matches(got, c["expect"])
        return {"t0": t0, "t1": t1, "result": got, "error": err, "ok": ok}

    # ------------------------------------------------------------------ one repetition
    def play_rep(self, scene, k, rep):
        env = self.make(rep)
        n = len(rep["threads"])
        prepared = {(t, i): self.prepare(c) for t, th in enumerate(rep["threads"]) for i, c in enumerate(th)}
        import torch
        torch.cuda.synchronize()
        start = threading.Barrier(n + 1)
        rounds = threading.Barrier(n) if rep.get("barrier_rounds") else None
        done = {(t, i): threading.Event() for t, th in enumerate(rep["threads"]) for i in range(len(th))}
        records = [[None] * len(th) for th in rep["threads"]]
        finished = [threading.Event() for _ in range(n)]

        def work(t):
            try:
                start.wait()
                for i, c in enumerate(rep["threads"][t]):
                    if self.device_error.is_set():
                        return
                    self.progress[t] = [scene, k, i, c["op"], "waiting" if (c["after"] is not None or c["round"] is not None) else "calling"]
                    if c["round"] is not None and rounds is not None:
                        rounds.wait(DEADLINE_S)
                    if c["after"] is not None:
                        if not done[tuple(c["after"])].wait(DEADLINE_S):
                            return
                    self.progress[t][4] = "calling"
                    records[t][i] = self.record(env, c, prepared[(t, i)])
                    done[(t, i)].set()
                self.progress[t] = [scene, k, len(rep["threads"][t]), None, "done"]
            except threading.BrokenBarrierError:
                return
            finally:
                finished[t].set()

        self.progress = {t: [scene, k, 0, None, "start"] for t in range(n)}
        threads = [threading.Thread(target=work, args=(t,), daemon=True) for t in range(n)]
        for th in threads:
            th.start()
        start.wait()
        t_start = time.perf_counter_ns()
        deadline = time.monotonic() + DEADLINE_S
        for t in range(n):
            while not finished[t].wait(0.05):
                if self.device_error.is_set():
                    self.leave(4, "H2V_ERR_DEVICE in a thread")
                if time.monotonic() > deadline:
                    self.leave(3, "the deadline of %g s expired" % DEADLINE_S)
        if self.device_error.is_set():
            self.leave(4, "H2V_ERR_DEVICE in a thread")
        main = [self.record(env, c) for c in rep["main_after"]]
        if self.device_error.is_set():
            self.leave(4, "H2V_ERR_DEVICE on the main thread")
        # the first mismatching calls again, alone, on fresh objects of the same contexts
        replays = []
        for t, th in enumerate(rep["threads"]):
            for i, c in enumerate(th):
                if records[t][i] is not None and not records[t][i]["ok"] and len(replays) < REPLAYS and c["after"] is None:
                    replays.append({"thread": t, "index": i, "op": c["op"], "alone_ok": self.replay_alone(rep, env, t, i)})
        self.close(rep, env)
        return {"start": t_start, "threads": records, "main": main, "replays": replays}

    def replay_alone(self, rep, env, t, i):
        """thread t's calls up to call i, alone, on fresh copies of the objects they use -> is call i right now?"""
        calls = rep["threads"][t][:i + 1] if rep["threads"][t][i]["uses"] else [rep["threads"][t][i]]     # (a call on the context alone has no history)
        used = {name for c in calls for name in c["uses"]}
        fresh = dict(env)
        made = []
        try:
            for spec in rep["objects"]:
                if spec[0] in used:
                    fresh[spec[0]] = self.make_object(env, spec)
                    made.append(fresh[spec[0]])
            last = None
            for c in calls:
                last = self.record(fresh, c)
            return bool(last["ok"])
        finally:
            for obj in reversed(made):
                obj.close()

    def leave(self, code, why):
        with open(os.path.join(self.workdir, "stuck.json"), "w") as f:
            json.dump({"why": why, "progress": {str(t): p for t, p in self.progress.items()}}, f)
            f.flush()
            os.fsync(f.fileno())
        sys.stdout.flush()
        os._exit(code)

    def play(self, scene):
        self.lib.scene = scene["name"]
        t0 = time.perf_counter()
        reps = [self.play_rep(scene["name"], k, rep) for k, rep in enumerate(scene["reps"])]
        out = {"name": scene["name"], "seconds": time.perf_counter() - t0, "reps": reps, "symbols": self.lib.report(scene["name"])}
        with open(os.path.join(self.workdir, scene["name"] + ".json"), "w") as f:
            json.dump(out, f)


def main(workdir):
    with open(os.path.join(workdir, "scenes.pkl"), "rb") as f:
        data = pickle.load(f)
    player = Player(workdir, data)
    only = sys.argv[2].split(",") if len(sys.argv) > 2 else None
    for scene in data["scenes"]:
        if only is None or scene["name"] in only:
            player.play(scene)
            print("%-14s %.2f s" % (scene["name"], json.load(open(os.path.join(workdir, scene["name"] + ".json")))["seconds"]), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
