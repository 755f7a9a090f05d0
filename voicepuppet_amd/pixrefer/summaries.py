"""TensorBoard summaries of a PixReferNet training step, the images PNG-encoded on the device.

What the reference's merged summary op writes at every summary step (train_pixrefer.py:101-132, 146): three scalars and five image
summaries of up to three images each, under the tags tf.summary.image gives them inside the reference's name scopes.  Here the five
sources are the step's own device tensors; the encodes (voicepuppet_amd/png.py) are enqueued on the step's stream, and the host copies
only the PNG bytes.
"""
from .._handle import rows_to_host
from ..png import PngEncoder
from ..utils.tb_events import EventFileWriter

SCALAR_TAGS = ("discriminator_loss", "generator_loss_GAN", "generator_loss_L1")
IMAGE_NAMES = ("inputs1", "targets", "outputs", "alphas", "inputs0")      # the order of train_pixrefer.py:105-118
MAX_OUTPUTS = 3                                                            # tf.summary.image's default


def image_tag(name, i):
  return "%s_summary/%s/image/%d" % (name, name, i)


class TrainSummaries:
  """enqueue(engine) right behind a training step -> the pending encodes; write(step, scalars, pending) -> one Event in
  logdir/events.out.tfevents.*.  The sources have to stay unchanged until the encodes have run: enqueue before the next batch is drawn."""

  def __init__(self, logdir, batch, img_size):
    self.k = min(int(batch), MAX_OUTPUTS)
    self.size = int(img_size)
    self.encoder = PngEncoder(self.k, self.size, self.size, channels=3)
    self.writer = EventFileWriter(logdir)

  def sources(self, engine):
    """(name, tensor, channel offset) of the five summaries, from the engine's last step"""
    (inputs, _, targets), _ = engine._keep
    return (("inputs1", inputs, 3), ("targets", targets, 0), ("outputs", engine.fetch("Outputs"), 0), ("alphas", engine.fetch("Alphas"), 0),
            ("inputs0", inputs, 0))

  def enqueue(self, engine):
    return [(name,) + self.encoder.encode(t, channel_offset=off, frames=self.k) for name, t, off in self.sources(engine)]

  def collect(self, pending):
    """One wait for the 5 k lengths, then one for the used part of the rows -> {tag: (height, width, 3, png bytes)}"""
    images = {}
    for (name, _, _), (a, n) in zip(pending, rows_to_host([(rows, lengths) for _, rows, lengths in pending])):
      for i in range(self.k):
        images[image_tag(name, i)] = (self.size, self.size, 3, a[i, :n[i]].tobytes())
    return images

  def write(self, step, scalars, pending):
    self.writer.add_summary(step, dict(zip(SCALAR_TAGS, scalars)), self.collect(pending))
    self.writer.flush()

  def close(self):
    self.writer.close()
