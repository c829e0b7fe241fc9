"""What the native library prints: its trace lines go to file descriptor 2 from C++, past
sys.stderr, and its switches are read from the environment at every call."""
import contextlib
import os
import tempfile


@contextlib.contextmanager
def stderr_of_the_library(env):
    """Run the body with `env` set and file descriptor 2 in a file; yields a list that holds the text
    afterwards."""
    out = []
    old = {k: os.environ.get(k) for k in env}
    with tempfile.TemporaryFile(mode="w+b") as f:
        keep = os.dup(2)
        os.environ.update(env)
        os.dup2(f.fileno(), 2)
        try:
            yield out
        finally:
            os.dup2(keep, 2)
            os.close(keep)
            for k, v in old.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v
            f.seek(0)
            out.append(f.read().decode("utf-8", "replace"))
